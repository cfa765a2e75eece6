"""The Cellpose flow -> mask kernels on both sides of their switches (tests/dynamics_limits.py) on the device: seeds and
growth on a programmable histogram, the size floor and ceiling on every path, the three diffusion classes, the hole
kernels on and past their LDS tile and with nested labels -- labels and counts bit for bit against
oracle/cellpose_dynamics.py, flow errors within rtol 1e-9 / atol 1e-12; every case alone and as plane 1 of a two-plane
call; then everything once more in a child process under AMT_DEBUG_POISON=1 -- no mismatch, no dirty scratch padding, every
output digest equal to the in-process run's.  tests/test_host_dynamics_limits.py shows which side of which switch each case
is on.

Findings these cases pin (reverting the fix fails the named case):
  "ceiling 19 20 21 of 2000 x 0.01" (both paths): the size ceiling was int(n * float32(fraction)) = 19, the oracle's 20;
  "labels 1 3 6, nlabels 6, max_label 9": amt_cellpose_flow_error handed out the error slots above nlabels unwritten;
  "a value above max_label" (fill 1): a flagged plane kept such a value and indexed the keep flags with it."""
import pytest

import dynamics_limits as dl
import poison_child

pytestmark = pytest.mark.gpu

# the child's time limit: ten times the in-process run on an MI355X, rounded up to a whole minute
# (profiles/dynamics_limits.json: 3.3 s measured, references included; 33 s -> 60 s)
CHILD_TIMEOUT_S = 60

_RESULTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _group(ctx, group):
    """The in-process run of one group: made once, shared with the poison test."""
    if group not in _RESULTS:
        _RESULTS[group] = dl.run(ctx, [group])
    return _RESULTS[group]


def _mismatches(records):
    return [(r["op"], r["param"], tuple(r["shape"]), r["variant"], r["index"]) for r in records if r["status"] != "pass"]


@pytest.mark.parametrize("group", dl.GROUPS)
def test_group_matches_its_references(ctx, group):
    res = _group(ctx, group)
    assert res["records"], group
    bad = _mismatches(res["records"])
    assert not bad, f"{len(bad)} of {len(res['records'])} cases differ from their reference; the first: {bad[:10]}"


def test_every_case_ran_alone_and_in_a_batch(ctx):
    ran = {}
    for g in dl.GROUPS:
        for r in _group(ctx, g)["records"]:
            ran.setdefault((r["group"], r["param"]), set()).add(r["variant"])
    assert not dl.EXCLUDED and set(ran) == {(c["group"], c["name"]) for c in dl.cases()}
    for c in dl.cases():
        want = {"single", "batch"} if len(c["planes"]) == 1 else {"single"} | {f"plane {i} alone" for i in range(len(c["planes"]))}
        assert ran[(c["group"], c["name"])] == want, c["name"]


def _key(r):
    return (r["group"], r["op"], r["param"], tuple(r["shape"]), r["variant"])


def test_everything_under_poison(ctx, tmp_path):
    out = tmp_path / "dynamics.json"
    res = poison_child.run_module("tests.dynamics_limits", out, CHILD_TIMEOUT_S, "the poisoned run")
    bad = _mismatches(res["records"])
    assert not bad, f"{len(bad)} cases differ from their reference under poison; the first: {bad[:10]}"
    assert not res["dirty"], f"{len(res['dirty'])} scratch checks came back dirty; the first: {res['dirty'][:5]}"
    here = {}
    for g in dl.GROUPS:
        here.update({_key(r): r["sha256"] for r in _group(ctx, g)["records"]})
    there = {_key(r): r["sha256"] for r in res["records"]}
    poison_child.assert_unmoved(here, there)
