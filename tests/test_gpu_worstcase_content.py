"""Worst-case content (tests/worstcase_content.py) on the device: labelling, EDT, peak markers, the watershed by its three
routes, expand_labels, the flood-class limits, marker labels at 16 bits and the single-heap emulation beyond its LDS slots,
bit for bit against the references of the operators' own tests; then everything once more in a child process under
AMT_DEBUG_POISON=1 -- no mismatch, no dirty scratch padding, every output digest equal to the in-process run's.
tests/test_host_worstcase_content.py shows which side of which switch each input is on."""
import pytest

import poison_child
import worstcase_content as wc

pytestmark = pytest.mark.gpu

# the child's time limit: ten times the in-process run on an MI355X, rounded up to a whole minute
# (profiles/worstcase_content.json: 4.3 s measured, references included)
CHILD_TIMEOUT_S = 60

_RESULTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _group(ctx, group):
    """The in-process run of one group: made once, shared with the poison test."""
    if group not in _RESULTS:
        _RESULTS[group] = wc.run(ctx, [group])
    return _RESULTS[group]


def _mismatches(records):
    return [(r["op"], r["param"], tuple(r["shape"]), r["variant"], r["index"]) for r in records if r["status"] != "pass"]


@pytest.mark.parametrize("group", wc.GROUPS)
def test_group_matches_its_references(ctx, group):
    res = _group(ctx, group)
    assert res["records"], group
    bad = _mismatches(res["records"])
    assert not bad, f"{len(bad)} of {len(res['records'])} cases differ from their reference; the first: {bad[:10]}"


def test_every_listed_operator_ran_on_every_pattern_and_shape(ctx):
    ran = set()
    for g in wc.GROUPS[:6]:
        ran |= {(r["op"].split()[0] if r["op"].startswith("label ") else r["op"], r["param"].split()[0], tuple(r["shape"]))
                for r in _group(ctx, g)["records"] if r["variant"] == "single"}
    want = {(op, n, s) for op in wc.LABEL_OPS + wc.WATERSHED_OPS for n in wc.PATTERNS for s in wc.SHAPES}
    assert not wc.EXCLUDED and want <= ran, sorted(want - ran)[:10]


def _key(r):
    return (r["group"], r["op"], r["param"], tuple(r["shape"]), r["variant"])


def test_everything_under_poison(ctx, tmp_path):
    out = tmp_path / "worstcase.json"
    res = poison_child.run_module("tests.worstcase_content", out, CHILD_TIMEOUT_S, "the poisoned run")
    bad = _mismatches(res["records"])
    assert not bad, f"{len(bad)} cases differ from their reference under poison; the first: {bad[:10]}"
    assert not res["dirty"], f"{len(res['dirty'])} scratch checks came back dirty; the first: {res['dirty'][:5]}"
    here = {}
    for g in wc.GROUPS:
        here.update({_key(r): r["sha256"] for r in _group(ctx, g)["records"]})
    there = {_key(r): r["sha256"] for r in res["records"]}
    poison_child.assert_unmoved(here, there)
