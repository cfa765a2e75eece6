"""The integer tables of prefix_codes_kernel (``_thresholds.prefix_rule_tables``) against the float64 rule they restate
(``_thresholds.prefix_rule``): bin, ``above`` and ``undecided`` of every sample, on ranges chosen to break a restatement
-- the unit range, a range across a binade boundary, ranges of 16 and of one grey level, ranges of a few ulps where
consecutive edges share a prefix and every sample is undecided -- and on samples placed at every edge and centre prefix
and beside it, with the low words at which the four integer forms change."""
import numpy as np
import pytest

from arcadia_microscopy_tools_amd._thresholds import prefix_classify, prefix_rule, prefix_rule_tables

_ULP1 = float(np.spacing(1.0))
RANGES = [
    (0.0, 1.0),
    (0.0, 0.37),
    (0.24, 0.51),  # 0.25 and 0.5 inside: edges on both sides of two binade boundaries
    (0.4999, 0.5001),
    (1000 / 65535, 1016 / 65535),  # 16 grey levels
    (1000 / 65535, 1001 / 65535),  # one grey level
    (0.015259021896696421, 0.015259021896696421 + 3e-9),
    (1.0, 1.0 + 40 * _ULP1),  # fewer distinct doubles than bins: every sample undecided
    (0.25 - 8 * float(np.spacing(0.2)), 0.25 + 8 * float(np.spacing(0.25))),
]
LOW_WORDS = np.array([0, 1, 0x7FFFFFFF, 0xFFFFFFFE, 0xFFFFFFFF], np.uint64)


def _samples(lo, hi, seed):
    """Doubles around [lo, hi]: every edge and centre prefix - 1, + 0, + 1 with the low words above, and 200,000 random
    ones (uniform in value and uniform in bit pattern, a little beyond either end)."""
    edges = np.linspace(lo, hi, 257)
    centres = (edges[:-1] + edges[1:]) / 2.0
    heads = np.concatenate([edges, centres]).view(np.uint64) >> np.uint64(32)
    heads = np.concatenate([np.maximum(heads, 1) - np.uint64(1), heads, heads + np.uint64(1)])
    adversarial = ((heads[:, None] << np.uint64(32)) | LOW_WORDS[None, :]).ravel()
    rng = np.random.default_rng(seed)
    blo, bhi = np.array([lo, hi]).view(np.uint64)
    margin = np.uint64(3) << np.uint64(32)
    bits = rng.integers(int(max(blo, margin) - margin), int(bhi + margin), 100_000, dtype=np.uint64)
    values = rng.uniform(lo, hi, 100_000).view(np.uint64)
    return np.concatenate([adversarial, bits, values]).view(np.float64)


@pytest.mark.parametrize("k", range(len(RANGES)))
def test_tables_equal_float64_rule(k):
    lo, hi = RANGES[k]
    v = _samples(lo, hi, seed=k)
    assert v.size >= 200_000 and (v >= 0).all() and np.isfinite(v).all()
    want = prefix_rule(v, lo, hi)
    tables = prefix_rule_tables(lo, hi)
    assert tables.shape == (257, 4) and tables.dtype == np.uint32
    got = prefix_classify((v.view(np.uint64) >> np.uint64(32)).astype(np.uint32), tables)
    for name, g, w in zip(("bin", "above", "undecided"), got, want):
        assert np.array_equal(g, w), (k, name, int((g != w).sum()))
    print(f"range {k}: {v.size} samples, undecided share {want[2].mean():.3g}, bins used {np.unique(want[0]).size}")


def test_every_sample_undecided_on_a_range_of_a_few_ulps():
    lo, hi = RANGES[7]
    v = _samples(lo, hi, seed=0)
    inside = (v >= lo) & (v <= hi)
    assert prefix_rule(v, lo, hi)[2][inside].all()


@pytest.mark.parametrize("k", range(len(RANGES)))
def test_ae_is_non_decreasing(k):
    """The walk to max{i : p >= AE[i]} needs a sorted AE, also where consecutive edges share a prefix."""
    ae = prefix_rule_tables(*RANGES[k])[:, 0].astype(np.int64)
    assert (np.diff(ae) >= 0).all() and ae[0] == 0 and ae[-1] == 0xFFFFFFFF
    if k in (6, 7, 8):
        assert (np.diff(ae[1:256]) == 0).any()  # shared prefixes do occur on these ranges
