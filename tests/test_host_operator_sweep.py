"""The operator sweep's table (tests/operator_sweep.py) without a GPU: it builds, every reference runs on every shape that
is not excluded, and the conditions on EXCLUDED hold."""
import numpy as np

import operator_sweep as sw


def test_table_builds():
    assert len({o.name for o in sw.OPS}) == len(sw.OPS)
    assert {o.family for o in sw.OPS} == set(sw.FAMILIES)
    for o in sw.OPS:
        assert o.params and len(o.shapes()) >= 10, o.name
    # the shapes the issue names, each on one side of a switch of today's dispatch
    assert len(sw.SHAPES) == 16 and (70, 131) in sw.SHAPES and sw.PERCENTILE_SHAPES == [(255, 257), (256, 256)]
    assert 255 * 257 == 65535 and 256 * 256 == 65536
    radii = [int(4.0 * s + 0.5) for s in sw.SIGMAS]
    assert radii == [2, 8, 12, 13, 16]


def test_excluded_pairs_are_few_and_reasoned():
    sw.check_table()


def test_every_reference_runs_on_every_shape():
    n = 0
    for o in sw.OPS:
        for shape in o.shapes():
            for pi, p in enumerate(o.params):
                for kind in sw.kinds_checked(o):
                    want = sw.reference(o, pi, shape, kind)
                    assert isinstance(want, tuple) and len(want) >= 1, (o.name, p, shape, kind)
                    n += 1
    assert n > 10000
    # planes are read-only once made: a reference is computed once and shared
    ins = sw.inputs(sw.OPS[0], 0, (7, 5), 0)
    assert all(not a.flags.writeable for a in ins)


def test_rules():
    a = np.array([[1.0, np.nan], [3.0, 4.0]])
    assert sw.exact(a, a.copy()) == (True, None)
    b = a.copy()
    b[1, 0] = 3.0000001
    assert sw.exact(a, b) == (False, (1, 0))
    assert sw.close(1e-6, 0)(a, b)[0] and not sw.close(1e-9, 0)(a, b)[0]
    assert not sw.exact(a, a[:1])[0]
    # masked_sums: a sum off by one ulp of a large total is inside n 2^-53 sum|x|, a wrong count is not
    want = np.array([100.0, 10, 50.0, 5, 150.0])
    assert sw._masked_sums_rule(np.array([100.0 + 2 ** -46, 10, 50.0, 5]), want)[0]
    assert not sw._masked_sums_rule(np.array([100.0, 11, 50.0, 5]), want)[0]
    assert not sw._masked_sums_rule(np.array([100.0 + 1e-9, 10, 50.0, 5]), want)[0]
