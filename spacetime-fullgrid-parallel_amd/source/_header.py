"""A strict reader of include/stk.h: the header's text in, plain records out.

It covers the declaration forms that header uses and no more (prototypes, `typedef struct { ... } name;`,
function-pointer typedefs, opaque handles, object-like integer `#define`s) and raises HeaderError, quoting the text,
for anything else: what it cannot read it never skips.  _lib.py builds the ctypes binding from these records;
tests/test_binding_host.py lets the C compiler judge the reading against the real header.
"""
import re
from collections import namedtuple

# const: one flag for the base type and one per `*`, left to right
Type = namedtuple('Type', 'base stars const')
Param = namedtuple('Param', 'name type')
Function = namedtuple('Function', 'name ret params')
Header = namedtuple('Header', 'functions structs callbacks handles constants')

SCALARS = ('int', 'int32_t', 'int64_t', 'double')
POINTEES = ('void', 'char', 'unsigned char', 'uint8_t', 'uint16_t', 'uint32_t')  # behind a `*` only

_STARS = r'((?:\*\s*(?:const\b\s*)?)*)'
_DIRECTIVES = (r'#ifndef (\w+)\n#define \1', r'#include <stdint\.h>', r'#ifdef __cplusplus\nextern "C" \{\n#endif',
               r'#ifdef __cplusplus\n\}\n#endif', r'#endif', r'#define[ \t]+\w+\(.*')


class HeaderError(ValueError):
    pass


def c_spelling(t):
    """The type record as C text."""
    return ('const ' if t.const[0] else '') + t.base + ' ' + ''.join('*const ' if c else '*' for c in t.const[1:])


def parse(text):
    functions, structs, callbacks, handles, constants = [], [], {}, [], {}
    struct_names, seen = set(), set()

    def declarators(decl, where, named=True):
        """`const T *a, *const *b` -> [(name, Type)], every base type known."""
        m = re.fullmatch(r'(const\s+)?(unsigned char|\w+)\b\s*(.*)', decl.strip(), re.S)
        out = []
        for d in m.group(3).split(',') if m else [None]:
            dm = m and re.fullmatch(_STARS + (r'(\w+)' if named else r'(\w*)'), d.strip())
            if not dm:
                raise HeaderError('unrecognised declarator %r in: %s' % (decl.strip(), where))
            base, ptr = m.group(2), re.sub(r'\s', '', dm.group(1))
            by_value = base in SCALARS or base in callbacks
            if not (by_value or base in POINTEES or base in struct_names or base in handles) or not (by_value or ptr):
                raise HeaderError('unrecognised type %r in: %s' % (decl.strip(), where))
            const = (bool(m.group(1)),) + tuple(p.startswith('const') for p in ptr.split('*')[1:])
            out.append((dm.group(2), Type(base, len(const) - 1, const)))
        return out

    def function(name, ret, params, where):
        ret = declarators(ret, where, named=False)
        if len(ret) != 1 or ret[0][0]:
            raise HeaderError('unrecognised return type in: %s' % where)
        params = [] if params.strip() == 'void' else [
            Param(*declarators(p, where, named=False)[0]) for p in params.split(',')]
        return Function(name, ret[0][1], params)

    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    text = re.sub(r'^#define[ \t]+(\w+)[ \t]+(-?(?:0|[1-9]\d*))[ \t]*$',
                  lambda m: constants.update({m.group(1): int(m.group(2))}) or '', text, flags=re.M)
    for directive in _DIRECTIVES:
        text = re.sub(r'^%s[ \t]*$' % directive, '', text, flags=re.M)
    # split at the `;` outside braces: every piece must be one whole declaration
    *chunks, tail = re.split(r';(?![^{}]*\})', text)
    if tail.strip():
        raise HeaderError('unrecognised text: %s' % tail.strip())
    for chunk in chunks:
        where = ' '.join(chunk.split())
        if m := re.fullmatch(r'typedef struct \{(.*)\} (?P<name>\w+)', where):
            *lines, end = m.group(1).split(';')
            if end.strip():
                raise HeaderError('unrecognised text %r in: %s' % (end.strip(), where))
            structs.append((m['name'], [f for line in lines for f in declarators(line, where)]))
            struct_names.add(m['name'])
        elif m := re.fullmatch(r'typedef struct (?P<name>\w+) (?P=name)', where):
            handles.append(m['name'])
        elif m := re.fullmatch(r'typedef ([^()]+)\( ?\* ?(?P<name>\w+) ?\) ?\(([^()]*)\)', where):
            callbacks[m['name']] = function(m['name'], m.group(1), m.group(3), where)
        elif m := re.fullmatch(r'([^()]+?)\b(?P<name>\w+) ?\(([^()]*)\)', where):
            functions.append(function(m['name'], m.group(1), m.group(3), where))
        if not m or m['name'] in seen:
            raise HeaderError('%s: %s' % ('declared twice' if m else 'unrecognised text', where))
        seen.add(m['name'])
    return Header(functions, structs, callbacks, handles, constants)
