"""The ctypes binding is derived from include/stk.h (source/_header.py reads the
header, source/_lib.py maps the records to ctypes); here the C compiler judges
the derivation.  From header TEXT a C file is generated that includes the REAL
header and states, as static assertions and typed function pointers, what the
binding believes: it compiles exactly when the two agree.  No GPU, no ROCm and no
libstk.so are needed (the header includes <stdint.h> alone); only the last test
loads the library."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG, REPO

from source import _header, _lib
from source._header import Function, Param, Type

HEADER = open(os.path.join(REPO, 'include', 'stk.h')).read()


def binding_check(text, tmp_path):
    """Reads `text`, derives the binding and compiles its claims against the real
    include/stk.h: (compiler's return code, its output, functions, structs checked)."""
    if not shutil.which('gcc'):
        pytest.skip('gcc missing')
    header = _header.parse(text)
    structs, prototypes, _ = _lib.bind(text)
    spell = _header.c_spelling
    out = ['#include <stddef.h>', '#include "stk.h"']

    def claim(cond, what):
        out.append('_Static_assert(%s, "%s");' % (cond, what))

    def pointer(rec, value, ctypes_types=None):
        params = [spell(p.type) for p in rec.params]
        out.append('static %s(*const p_%s)(%s) __attribute__((unused)) = %s;' % (
            spell(rec.ret), rec.name, ', '.join(params) or 'void', value))
        if ctypes_types is None:  # a callback without a Python type: passed as an address
            return
        assert len(ctypes_types) == 1 + len(params), rec.name
        for i, (c, t) in enumerate(zip([spell(rec.ret)] + params, ctypes_types)):
            claim('sizeof(%s) == %d' % (c, ctypes.sizeof(t)),
                  '%s: width of %s' % (rec.name, 'parameter %d' % i if i else 'the result'))

    for name, fields in header.structs:
        cls = structs[name]
        claim('sizeof(%s) == %d' % (name, ctypes.sizeof(cls)), 'sizeof %s' % name)
        for f, _ in fields:
            claim('offsetof(%s, %s) == %d' % (name, f, getattr(cls, f).offset), 'offset of %s.%s' % (name, f))
            claim('sizeof(((%s *)0)->%s) == %d' % (name, f, getattr(cls, f).size), 'size of %s.%s' % (name, f))
    for f in header.functions:
        res, args = prototypes[f.name]
        pointer(f, f.name, [res] + args)
    for name, rec in header.callbacks.items():
        fn = _lib.CALLBACKS.get(name)  # the hand-written Python types: argument count and widths
        pointer(rec, '(%s)0' % name, fn and [fn._restype_] + list(fn._argtypes_))
    src = tmp_path / 'binding_check.c'
    src.write_text('\n'.join(out) + '\n')
    res = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-I' + os.path.join(REPO, 'include'), '-c', str(src),
                          '-o', str(tmp_path / 'binding_check.o')], capture_output=True, text=True)
    return res.returncode, res.stdout + res.stderr, len(header.functions), len(header.structs)


def test_the_compiler_accepts_the_derived_binding(tmp_path):
    rc, log, n_functions, n_structs = binding_check(HEADER, tmp_path)
    assert rc == 0, log[:4000]
    header = _header.parse(HEADER)
    types = {name for name, _ in header.structs} | set(header.handles) | set(header.callbacks)
    independent = set(re.findall(r'\b(stk_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', ' ', HEADER, flags=re.S))) - types
    assert n_functions == len(independent) == len(_lib.EXPORTED_SYMBOLS) and independent == set(_lib.EXPORTED_SYMBOLS)
    assert n_structs == 8 and {name for name, _ in header.structs} == set(_lib.STRUCT_NAMES)
    for name in _lib.STRUCT_NAMES.values():
        assert issubclass(getattr(_lib, name), ctypes.Structure) and getattr(_lib, name).__name__ == name


@pytest.mark.parametrize('old, new, where', [
    # int64_t M, int32_t n_cols of the history scan swapped
    ('void *stream, int64_t M, int32_t n_cols, const double *u,',
     'void *stream, int32_t n_cols, int64_t M, const double *u,', 'p_stk_history_scan'),
    # an int32_t parameter of the prolongation turned into int64_t
    ('const stk_transfer_plan *plan, int32_t a,', 'const stk_transfer_plan *plan, int64_t a,',
     'p_stk_transfer_prolong'),
    # one parameter of the solidification scan removed
    ('stk_solid_plan *plan, int64_t M, int32_t n_cols,', 'stk_solid_plan *plan, int64_t M,', 'p_stk_solid_scan'),
    # a field of stk_mg_level removed
    ('    const stk_ell_rows *ell_ra;\n', '', 'offsetof(stk_mg_level, ell_fwd0)'),
    # count and peer of stk_comm_msg swapped
    ('    int64_t count; /* doubles */\n    int32_t peer;  /* rank */\n', '    int32_t peer;\n    int64_t count;\n',
     'offsetof(stk_comm_msg, count)'),
    # int32_t M, K; of stk_pack_pattern reduced to int32_t M;
    ('    int32_t M, K;\n    int32_t col_bits;', '    int32_t M;\n    int32_t col_bits;',
     'offsetof(stk_pack_pattern, col_bits)'),
    # the return type of the sum over the steps turned into int
    ('double stk_sum_steps', 'int stk_sum_steps', 'p_stk_sum_steps'),
], ids=['swapped-pair', 'widened-int32', 'parameter-removed', 'field-removed', 'fields-swapped', 'declarator-removed',
        'return-type'])
def test_the_compiler_refuses_a_misread_header(tmp_path, old, new, where):
    """The reader is handed altered text, the compiler the real header: each
    alteration is a row of the old hand-kept table gone wrong."""
    assert HEADER.count(old) == 1, old
    rc, log, _, _ = binding_check(HEADER.replace(old, new), tmp_path)
    assert rc != 0 and 'error' in log and where in log, log[:2000]


@pytest.mark.parametrize('text, named', [
    ('int stk_f(void *stream, float x);', 'stk_f'),
    ('int stk_f(unsigned n);', 'stk_f'),
    ('int stk_f(long n);', 'stk_f'),
    ('int stk_f(size_t n);', 'stk_f'),
    ('int stk_f(double a[3]);', 'stk_f'),
    ('typedef struct { int32_t n; } stk_s;\nint stk_f(stk_s s);', 'stk_f'),
    ('int stk_f(int32_t n, ...);', 'stk_f'),
    ('typedef struct {\n    int32_t flag : 1;\n} stk_s;', 'stk_s'),
    ('typedef union {\n    int32_t i;\n    double d;\n} stk_u;', 'stk_u'),
    ('int stk_f(int32_t n)\nint stk_g(int32_t m);', 'stk_f'),   # a missing `;`
    ('typedef struct stk_x stk_x\nint stk_f(stk_x *x);', 'stk_x stk_x'),
    ('typedef struct {\n    int32_t n\n    double d;\n} stk_s;', 'stk_s'),
], ids=['float', 'unsigned', 'long', 'size_t', 'array', 'struct-by-value', 'ellipsis', 'bit-field', 'union',
        'missing-semicolon', 'missing-semicolon-typedef', 'missing-semicolon-field'])
def test_the_reader_refuses_what_it_has_no_rule_for(text, named):
    with pytest.raises(_header.HeaderError) as err:
        _header.parse(text)
    assert named in str(err.value), str(err.value)


@pytest.mark.parametrize('text', [
    'int stk_f(void);\nstray\nint stk_g(void);',
    'int stk_f(void);\n#pragma once\nint stk_g(void);',
    'int stk_f(void);\n#define STK_N 3 + 4\nint stk_g(void);',
    'int stk_f(void);\n#define STK_N 010\nint stk_g(void);',   # 8 in C, 10 to int(): neither is read
    'int stk_f(void);\n#define STK_N 0x10\nint stk_g(void);',
    'int stk_f(void);\nint stk_g(void)',
    'int stk_f(void);\n}\n',
])
def test_the_reader_leaves_no_text_unread(text):
    with pytest.raises(_header.HeaderError, match='unrecognised'):
        _header.parse(text)
    assert len(_header.parse('int stk_f(void);\nint stk_g(void);').functions) == 2


@pytest.mark.parametrize('text, named', [
    ('int stk_f(void);\nint stk_g(void);\nint stk_f(int32_t n);', 'stk_f(int32_t n)'),
    ('typedef struct { int32_t n; } stk_s;\ntypedef struct { double d; } stk_s;', 'double d'),
    ('typedef struct stk_x stk_x;\ntypedef struct stk_x stk_x;', 'stk_x'),
    ('typedef int (*stk_cb)(void *ctx);\ntypedef int (*stk_cb)(void *ctx, int32_t n);', 'int32_t n'),
    ('typedef struct stk_x stk_x;\nint stk_x(void);', 'stk_x(void)'),
])
def test_the_reader_refuses_a_name_declared_twice(text, named):
    with pytest.raises(_header.HeaderError, match='declared twice') as err:
        _header.parse(text)
    assert named in str(err.value)


def test_declaration_forms():
    T = Type
    h = _header.parse('''/* a comment with a declaration in it: int stk_not(void); */
#ifndef STK_H
#define STK_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define STK_N 7
#define STK_ROWS(d) (6 + 2 * (d))
typedef struct stk_x stk_x;
typedef struct {
    int32_t M, K;             /* two declarators */
    const double *va, *const *vm; /* of different depth */
} stk_s;
typedef struct {
    const stk_s *first, *second;
    void *buf;
} stk_t;
typedef int (*stk_cb)(void *ctx, int32_t n);
int stk_create(int64_t n,
               const int32_t *const *p,
               stk_x **out);
int64_t stk_size(void);
const char *stk_name(double, stk_cb cb, const stk_t *);
#ifdef __cplusplus
}
#endif
#endif /* STK_H */
''')
    assert h.constants == {'STK_N': 7}
    assert h.handles == ['stk_x']
    assert h.structs == [
        ('stk_s', [('M', T('int32_t', 0, (False,))), ('K', T('int32_t', 0, (False,))),
                   ('va', T('double', 1, (True, False))), ('vm', T('double', 2, (True, True, False)))]),
        ('stk_t', [('first', T('stk_s', 1, (True, False))), ('second', T('stk_s', 1, (True, False))),
                   ('buf', T('void', 1, (False, False)))])]
    assert h.callbacks == {'stk_cb': Function('stk_cb', T('int', 0, (False,)), [
        Param('ctx', T('void', 1, (False, False))), Param('n', T('int32_t', 0, (False,)))])}
    assert h.functions == [
        Function('stk_create', T('int', 0, (False,)), [
            Param('n', T('int64_t', 0, (False,))), Param('p', T('int32_t', 2, (True, True, False))),
            Param('out', T('stk_x', 2, (False, False, False)))]),
        Function('stk_size', T('int64_t', 0, (False,)), []),
        Function('stk_name', T('char', 1, (True, False)), [
            Param('', T('double', 0, (False,))), Param('cb', T('stk_cb', 0, (False,))),
            Param('', T('stk_t', 1, (True, False)))])]
    assert [_header.c_spelling(p.type) for p in h.functions[0].params] == [
        'int64_t ', 'const int32_t *const *', 'stk_x **']


def test_the_mapping_to_ctypes():
    structs, prototypes, constants = _lib.bind('''#define STK_N 7
typedef struct stk_x stk_x;
typedef struct { int32_t n; const double *va; } stk_s;
typedef int (*stk_operator_fn)(void *ctx, void *stream, const double *x, double *y);
typedef int (*stk_other_fn)(void *ctx);
int stk_create(int64_t n, const int32_t *const *p, double **slab, stk_x **out);
double stk_apply(stk_x *x, const stk_s *s, stk_operator_fn f, stk_other_fn g, const char *key, int32_t v);
int stk_read(char *buf, const char *const *keys);
const char *stk_name(void);
''')
    c_p = ctypes.c_void_p
    assert constants == {'STK_N': 7}
    assert structs['stk_s']._fields_ == [('n', ctypes.c_int32), ('va', c_p)]
    assert prototypes == {
        'stk_create': (ctypes.c_int, [ctypes.c_int64, c_p, c_p, ctypes.POINTER(c_p)]),
        'stk_apply': (ctypes.c_double, [c_p, ctypes.POINTER(structs['stk_s']), _lib.OPERATOR_FN, c_p, ctypes.c_char_p,
                                        ctypes.c_int32]),
        'stk_read': (ctypes.c_int, [c_p, c_p]),  # only `const char *` is a string
        'stk_name': (ctypes.c_char_p, [])}


def test_a_header_the_reader_refuses_is_an_error_with_its_path(tmp_path, monkeypatch):
    monkeypatch.setattr(_lib, 'HEADER_PATH', str(tmp_path / 'stk.h'))
    with pytest.raises(_lib.StkError, match=re.escape(str(tmp_path / 'stk.h'))):
        _lib._bind_header()
    (tmp_path / 'stk.h').write_text('int stk_f(float x);\n')
    with pytest.raises(_lib.StkError, match=re.escape(str(tmp_path / 'stk.h'))) as err:
        _lib._bind_header()
    assert 'float x' in str(err.value)


def test_the_loaded_library_carries_the_derived_binding():
    if not os.path.exists(os.path.join(PKG, 'libstk.so')):
        pytest.skip('libstk.so missing')
    from source import history, transfer
    lib = _lib.lib()
    assert sorted(_lib.prototypes) == _lib.EXPORTED_SYMBOLS
    for name, (res, args) in _lib.prototypes.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert _lib.STK_TRANSFER_MAX_A == 8 == transfer.MAX_A
    assert _lib.STK_HISTORY_STATE == len(history.STATE_ROWS)
