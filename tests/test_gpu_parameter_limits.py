"""The parameter-limit table (tests/parameter_limits.py) on the device: every operator at both ends of its documented
parameter ranges and at each switch inside them against the reference of its own test, one refusal just outside each end,
amt_nn_affine_act_bf16 against its definition; then everything once more in a child process under AMT_DEBUG_POISON=1 -- no
mismatch, no dirty scratch padding, every output digest equal to the in-process run's.
tests/test_host_parameter_limits.py shows that each case sits on the end or switch it names."""
import pytest

import parameter_limits as pl
import poison_child

pytestmark = pytest.mark.gpu

# the child's time limit: ten times the in-process run on an MI355X, rounded up to a whole minute
# (profiles/parameter_limits.json: 13.5 s measured, references included)
CHILD_TIMEOUT_S = 180

_RESULTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _group(ctx, group):
    """The in-process run of one group: made once, shared with the completeness and the poison test."""
    if group not in _RESULTS:
        _RESULTS[group] = pl.run(ctx, [group])
    return _RESULTS[group]


def _mismatches(records):
    return [(r["op"], r["param"], tuple(r["shape"]), r["index"]) for r in records if r["status"] != "pass"]


@pytest.mark.parametrize("group", pl.GROUPS)
def test_group_matches_its_references(ctx, group):
    res = _group(ctx, group)
    assert res["records"], group
    bad = _mismatches(res["records"])
    assert not bad, f"{len(bad)} of {len(res['records'])} cases differ from their reference; the first: {bad[:10]}"


def test_every_range_has_both_ends(ctx):
    ran, called = set(), set()
    for g in pl.GROUPS:
        res = _group(ctx, g)
        ran |= {tuple(m) for r in res["records"] if r["status"] == "pass" for m in r["marks"]}
        called |= set(res["called"])
    want = set(pl.wanted_marks())
    assert not pl.EXCLUDED and want <= ran, sorted(want - ran)[:10]
    assert "amt_nn_affine_act_bf16" in called and "amt_threshold_value" in called and "amt_hist_u16" in called


def _key(r):
    return (r["group"], r["op"], r["param"], tuple(r["shape"]), r["variant"])


def test_everything_under_poison(ctx, tmp_path):
    out = tmp_path / "limits.json"
    res = poison_child.run_module("tests.parameter_limits", out, CHILD_TIMEOUT_S, "the poisoned run")
    bad = _mismatches(res["records"])
    assert not bad, f"{len(bad)} cases differ from their reference under poison; the first: {bad[:10]}"
    assert not res["dirty"], f"{len(res['dirty'])} scratch checks came back dirty; the first: {res['dirty'][:5]}"
    here = {}
    for g in pl.GROUPS:
        here.update({_key(r): r["sha256"] for r in _group(ctx, g)["records"]})
    there = {_key(r): r["sha256"] for r in res["records"]}
    poison_child.assert_unmoved(here, there)
