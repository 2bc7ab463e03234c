"""The contract of the history maps (include/stk.h "history maps", source/history.py) as a
NumPy loop -- the oracle of tests/test_history_gpu.py, which compares the device against it
with array_equal -- its properties, the column-chunk planner of the per-point form, and the
argument checks of the public call that need no device."""
import itertools
import types

import numpy as np
import pytest

from source.history import FIELDS, STATE_ROWS, THRESHOLD_FIELDS, check_arguments, history_maps, plan_chunks

PEAK, T_PEAK, DOSE, ABOVE, T_FIRST, T_LAST, MAX_RATE, MIN_RATE, LAST = range(9)


def numpy_history_scan(v, k_first, h, theta, state=None):
    """The contract, column by column over the rows of v (M, n_cols): returns the (9, M)
    state; state=None starts fresh at column 0, else the given state is carried on (and left
    unchanged).  Every operation is one NumPy operation on doubles: rounded on its own."""
    v = np.asarray(v, dtype=np.float64)
    M, n = v.shape
    h, theta = np.float64(h), np.float64(theta)
    first = 0
    if state is None:
        assert n >= 1
        tk = np.float64(float(k_first) * h)
        s = np.empty((9, M))
        s[PEAK] = s[LAST] = v[:, 0]
        s[T_PEAK] = tk
        s[DOSE] = s[ABOVE] = 0.0
        s[T_FIRST] = s[T_LAST] = np.where(v[:, 0] > theta, tk, np.nan)
        s[MAX_RATE], s[MIN_RATE] = -np.inf, np.inf
        first = 1
    else:
        s = np.array(state, dtype=np.float64)
    half_h = np.float64(0.5) * h
    with np.errstate(all='ignore'):  # the crossing is computed everywhere and used where there is one
        for c in range(first, n):
            k = k_first + c
            a, b = s[LAST].copy(), v[:, c]
            tk, te = np.float64(float(k) * h), np.float64(float(k - 1))
            higher = b > s[PEAK]
            s[PEAK] = np.where(higher, b, s[PEAK])
            s[T_PEAK] = np.where(higher, tk, s[T_PEAK])
            s[DOSE] = s[DOSE] + (a + b) * half_h
            rate = (b - a) / h
            s[MAX_RATE] = np.where(rate > s[MAX_RATE], rate, s[MAX_RATE])
            s[MIN_RATE] = np.where(rate < s[MIN_RATE], rate, s[MIN_RATE])
            a_up, b_up = a > theta, b > theta
            both, rising, falling = a_up & b_up, b_up & ~a_up, a_up & ~b_up
            x = (theta - a) / (b - a)
            crossing = (te + x) * h
            s[ABOVE] = np.where(both, s[ABOVE] + h, np.where(rising, s[ABOVE] + h * (1.0 - x),
                                                            np.where(falling, s[ABOVE] + h * x, s[ABOVE])))
            s[T_FIRST] = np.where(rising & np.isnan(s[T_FIRST]), crossing, s[T_FIRST])
            s[T_LAST] = np.where(both | rising, tk, np.where(falling, crossing, s[T_LAST]))
            s[LAST] = b
    return s


def scalar_history_scan(row, k_first, h, theta):
    """The same contract as the plain loop over one row, in Python floats (IEEE doubles)."""
    nan, inf = float('nan'), float('inf')
    h, theta = float(h), float(theta)
    v = float(row[0])
    tk = float(k_first) * h
    peak = last = v
    t_peak, dose, above = tk, 0.0, 0.0
    t_first = t_last = tk if v > theta else nan
    max_rate, min_rate = -inf, inf
    for c in range(1, len(row)):
        k = k_first + c
        a, b, e = last, float(row[c]), k - 1
        if b > peak:
            peak, t_peak = b, float(k) * h
        dose = dose + (a + b) * (0.5 * h)
        rate = (b - a) / h
        if rate > max_rate:
            max_rate = rate
        if rate < min_rate:
            min_rate = rate
        a_up, b_up = a > theta, b > theta
        if a_up and b_up:
            above += h
            t_last = float(k) * h
        elif b_up:
            x = (theta - a) / (b - a)
            above += h * (1.0 - x)
            if t_first != t_first:
                t_first = (float(e) + x) * h
            t_last = float(k) * h
        elif a_up:
            x = (theta - a) / (b - a)
            above += h * x
            t_last = (float(e) + x) * h
        last = b
    return np.array([peak, t_peak, dose, above, t_first, t_last, max_rate, min_rate, last])


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def planted_rows(rng, M, n, theta):
    """randn rows with the planted cases of the slab test: row 0 constant at theta, a row
    with exact ties of the maximum, a row of integers around an integer threshold's value
    (nodes exactly AT theta on either side of crossings), a monotone row."""
    v = rng.randn(M, n)
    v[0] = theta
    if M > 1:
        v[1] = np.where(np.arange(n) % 3 == 1, 7.5, v[1].clip(max=7.0))
    if M > 2:
        v[2] = np.round(theta) + np.array([(-1, 0, 1, 0, 0, -1, 1, 1, 0, -1)[c % 10] for c in range(n)])
    if M > 3:
        v[3] = np.sort(v[3])
    return v


def test_state_rows_and_fields():
    assert STATE_ROWS == FIELDS + ('last',) and len(STATE_ROWS) == 9
    assert STATE_ROWS.index('dose') == DOSE and STATE_ROWS.index('min_rate') == MIN_RATE
    assert THRESHOLD_FIELDS == ('time_above', 't_first', 't_last')


def test_vector_form_is_the_plain_loop():
    rng = np.random.RandomState(5)
    h, theta = 1.0 / 3.0, 0.3
    v = planted_rows(rng, 40, 23, theta)
    got = numpy_history_scan(v, 0, h, theta)
    for i in range(len(v)):
        assert same(got[:, i], scalar_history_scan(v[i], 0, h, theta)), i
    late = numpy_history_scan(v, 11, h, theta)
    assert same(late[:, 7], scalar_history_scan(v[7], 11, h, theta))


def test_chunked_with_carry_is_the_one_shot_scan():
    rng = np.random.RandomState(6)
    v, h, theta = rng.randn(50, 65), 1.0 / 64, 0.3
    whole = numpy_history_scan(v, 0, h, theta)
    state, at = None, 0
    for width in (1, 7, 2, 30, 25):
        state = numpy_history_scan(v[:, at:at + width], at, h, theta, state)
        at += width
    assert at == 65 and same(state, whole)
    # every split of 9 columns into two parts (the second part may not be empty: it is a call)
    v = planted_rows(rng, 30, 9, theta)
    whole = numpy_history_scan(v, 0, 0.125, theta)
    for cut in range(1, 9):
        first = numpy_history_scan(v[:, :cut], 0, 0.125, theta)
        kept = first.copy()
        assert same(numpy_history_scan(v[:, cut:], cut, 0.125, theta, first), whole), cut
        assert same(first, kept)  # the carried state is not changed in place
    assert same(numpy_history_scan(v[:, :0], 9, 0.125, theta, whole), whole)  # no column: untouched


def test_peak_dose_and_rates_are_what_numpy_says():
    rng = np.random.RandomState(7)
    v, h = rng.randn(64, 65), 1.0 / 64
    s = numpy_history_scan(v, 0, h, 0.3)
    assert same(s[PEAK], v.max(axis=1)) and same(s[T_PEAK], v.argmax(axis=1) * h)
    trapezoid = getattr(np, 'trapezoid', None) or np.trapz
    assert np.allclose(s[DOSE], trapezoid(v, dx=h, axis=1), rtol=1e-13, atol=1e-15)
    rates = np.diff(v, axis=1) / h
    assert same(s[MAX_RATE], rates.max(axis=1)) and same(s[MIN_RATE], rates.min(axis=1))
    assert same(s[LAST], v[:, -1])
    assert np.all((s[ABOVE] >= 0.0) & (s[ABOVE] <= 1.0))
    both = ~np.isnan(s[T_FIRST])
    assert np.all(s[T_FIRST][both] <= s[T_LAST][both]) and same(np.isnan(s[T_FIRST]), np.isnan(s[T_LAST]))


def test_ties_the_earliest_node_wins():
    v = np.array([[1.0, 3.0, 2.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 2.0, 2.0, 2.0]])
    s = numpy_history_scan(v, 0, 0.25, 10.0)
    assert same(s[PEAK], [3.0, 2.0]) and same(s[T_PEAK], [0.25, 0.0])
    assert same(s[MAX_RATE], [8.0, 0.0]) and same(s[MIN_RATE], [-12.0, 0.0])


def test_a_row_constant_at_the_threshold_is_never_above():
    s = numpy_history_scan(np.full((1, 9), 0.3), 0, 0.125, 0.3)
    assert s[ABOVE, 0] == 0.0 and np.isnan(s[T_FIRST, 0]) and np.isnan(s[T_LAST, 0])
    assert s[PEAK, 0] == 0.3 and s[T_PEAK, 0] == 0.0 and s[DOSE, 0] == 8 * ((0.3 + 0.3) * 0.0625)


def test_nodes_exactly_at_the_threshold():
    """theta = 1, h = 1/2.  Values AT theta are not above: a crossing that starts at theta
    has x = 0, one that ends at theta has x = 1."""
    v = np.array([[0.0, 1.0, 2.0, 1.0, 0.0],   # up through theta at node 1, down through it at node 3
                  [2.0, 1.0, 2.0, 2.0, 1.0]])  # above, touches theta at node 1, ends AT theta
    s = numpy_history_scan(v, 0, 0.5, 1.0)
    # row 0: [1, 2]: a = theta, x = 0: the whole element; [2, 3]: b = theta, x = 1: the whole element
    assert s[ABOVE, 0] == 1.0 and s[T_FIRST, 0] == 0.5 and s[T_LAST, 0] == 1.5
    # row 1: above at node 0 (t_first = 0); [0, 1] falling x = 1; [1, 2] rising x = 0 (t_first stays);
    # [2, 3] both; [3, 4] falling to theta, x = 1, t_last = (3 + 1) h
    assert s[ABOVE, 1] == 2.0 and s[T_FIRST, 1] == 0.0 and s[T_LAST, 1] == 2.0


@pytest.mark.parametrize('n,h', [(65, 1.0 / 64), (9, 0.125)])
def test_infinite_thresholds(n, h):
    v = np.random.RandomState(8).randn(20, n)
    low, high = numpy_history_scan(v, 0, h, -np.inf), numpy_history_scan(v, 0, h, np.inf)
    assert np.all(low[ABOVE] == 1.0) and np.all(low[T_FIRST] == 0.0) and np.all(low[T_LAST] == 1.0)
    assert np.all(high[ABOVE] == 0.0) and np.all(np.isnan(high[T_FIRST])) and np.all(np.isnan(high[T_LAST]))
    for row in (PEAK, T_PEAK, DOSE, MAX_RATE, MIN_RATE, LAST):
        assert same(low[row], high[row])


# ---- the column chunks of the per-point form ---------------------------------------------------
@pytest.mark.parametrize('n_nodes,n_p,limit', [
    (65, 1, 256 << 20),            # one point: one chunk
    (65, 1 << 20, 256 << 20),      # the 1024^2 raster: 32 columns per chunk, 65 = 2 * 32 + 1
    (9, 5000, 8 * 5000),           # exactly one column fits
    (9, 5000, 100),                # not even one column fits: one column per chunk all the same
    (9, 1 << 40, 256 << 20),
    (10, 3, 8 * 3 * 4),            # N no multiple of the chunk
    (1, 7, 256 << 20),
    (33, 0, 256 << 20),
])
def test_plan_chunks_names_every_node_once_in_order(n_nodes, n_p, limit):
    chunks = plan_chunks(n_nodes, n_p, limit)
    assert list(itertools.chain.from_iterable(range(a, b) for a, b in chunks)) == list(range(n_nodes))
    for a, b in chunks:
        assert b - a >= 1 and ((b - a) * n_p * 8 <= limit or b - a == 1)
    widths = [b - a for a, b in chunks]
    assert all(w == widths[0] for w in widths[:-1]) and widths[-1] <= widths[0]


def test_plan_chunks_sizes():
    assert plan_chunks(65, 1) == [(0, 65)]
    assert plan_chunks(65, 1 << 20) == [(0, 32), (32, 64), (64, 65)]
    assert plan_chunks(9, 5000, 100) == [(k, k + 1) for k in range(9)]
    assert plan_chunks(10, 3, 96) == [(0, 4), (4, 8), (8, 10)]


# ---- argument checks that need no device ----------------------------------------------------------
def test_check_arguments():
    theta, names = check_arguments(None)
    assert theta == np.inf and names == ('peak', 't_peak', 'dose', 'max_rate', 'min_rate')
    assert check_arguments(0.5) == (0.5, FIELDS)
    assert check_arguments(-np.inf)[0] == -np.inf and check_arguments(np.inf)[1] == FIELDS
    assert check_arguments(1, np.zeros((4, 2)), 2, fields=('dose', 't_last')) == (1.0, ('dose', 't_last'))
    assert check_arguments(None, fields='peak')[1] == ('peak',)
    with pytest.raises(ValueError, match='threshold is NaN'):
        check_arguments(float('nan'))
    with pytest.raises(ValueError, match='temperature'):
        check_arguments(0.5, fields=('peak', 'temperature'))
    with pytest.raises(ValueError, match='needs a threshold'):
        check_arguments(None, fields=('time_above',))
    for bad in (np.zeros(4), np.zeros((4, 3)), np.zeros((2, 2, 2)), [1.0, 2.0]):
        with pytest.raises(ValueError, match='points of shape'):
            check_arguments(0.5, bad, 2)


def test_the_public_call_checks_before_it_touches_anything():
    """source.history.history_maps is the body of both drivers' history_maps(); with a
    vector of None it can only get as far as the checks."""
    mesh = types.SimpleNamespace(points=np.zeros((5, 2)))
    heat = types.SimpleNamespace(_sample_meshes=(mesh, None), sample_plan=None)
    with pytest.raises(ValueError, match='threshold is NaN'):
        history_maps(heat, None, threshold=float('nan'))
    with pytest.raises(ValueError, match='points of shape'):
        history_maps(heat, None, threshold=0.5, points=np.zeros((7, 3)))
    with pytest.raises(ValueError, match='fields must name'):
        history_maps(heat, None, threshold=0.5, fields=('heat',))
