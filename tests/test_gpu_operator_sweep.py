"""The operator sweep (tests/operator_sweep.py) on the device: every family against its references, every exported entry
point reached, and the whole table once more in a child process under AMT_DEBUG_POISON=1 -- scratch and allocations
poisoned, the padding behind every scratch buffer checked for stray writes, every output digest equal to the in-process
run's (a result must not depend on what the scratch held)."""
import pytest

import operator_sweep as sw
import poison_child

pytestmark = pytest.mark.gpu

# the child's time limit: ten times the in-process sweep on an MI355X, rounded up to a whole minute
# (profiles/operator_sweep.json: 10.6 s measured, references included)
CHILD_TIMEOUT_S = 120

# entry points the sweep need not reach, each with its reason; none of them reserves scratch
EXEMPT = {
    **{n: "context / stream plumbing" for n in ("amt_device_count", "amt_ctx_create", "amt_ctx_create_on_stream",
                                                "amt_ctx_destroy", "amt_ctx_set_fork", "amt_ctx_stream", "amt_last_error",
                                                "amt_version", "amt_device_name", "amt_stream_wait")},
    **{n: "memory helper" for n in ("amt_malloc", "amt_free", "amt_memcpy_h2d", "amt_memcpy_d2h", "amt_memcpy_d2d",
                                    "amt_memset", "amt_sync")},
    **{n: "event helper" for n in ("amt_event_create", "amt_event_record", "amt_event_wait", "amt_event_sync",
                                   "amt_event_destroy")},
    **{n: "timer helper" for n in ("amt_timer_create", "amt_timer_start", "amt_timer_stop", "amt_timer_elapsed_ms",
                                   "amt_timer_destroy")},
    **{n: "host helper (no GPU call)" for n in ("amt_host_alloc", "amt_host_copy", "amt_host_minmax_int",
                                                "amt_host_narrow_i64_i32", "amt_host_free")},
    "amt_debug_scratch_check": "the diagnostic call of the poison pass itself",
    "amt_nn_affine_act_bf16": "takes torch tensors; tests/parameter_limits.py compares it with its definition",
}

_RESULTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _family(ctx, family):
    """The in-process run of one family: made once, shared by the three tests."""
    if family not in _RESULTS:
        _RESULTS[family] = sw.run(ctx, [family])
    return _RESULTS[family]


def _mismatches(records):
    return [(r["op"], r["param"], tuple(r["shape"]), r["variant"], r["index"]) for r in records if r["status"] != "pass"]


@pytest.mark.parametrize("family", sw.FAMILIES)
def test_family_matches_its_references(ctx, family):
    res = _family(ctx, family)
    assert res["records"], family
    bad = _mismatches(res["records"])
    assert not bad, f"{len(bad)} of {len(res['records'])} cases differ from their reference; the first: {bad[:10]}"


def test_every_operator_is_reached(ctx):
    from arcadia_microscopy_tools_amd import _hip

    called = set()
    for family in sw.FAMILIES:
        called |= set(_family(ctx, family)["called"])
    exported = set(_hip.exported_names())
    assert set(EXEMPT) <= exported, sorted(set(EXEMPT) - exported)
    missing = exported - called - set(EXEMPT)
    assert not missing, f"entry points no case of the sweep calls: {sorted(missing)}"
    sw.check_table()


def _key(r):
    return (r["op"], r["param"], tuple(r["shape"]), r["variant"])


def test_sweep_under_poison(ctx, tmp_path):
    out = tmp_path / "sweep.json"
    res = poison_child.run_module("tests.operator_sweep", out, CHILD_TIMEOUT_S, "the poisoned sweep")
    bad = _mismatches(res["records"])
    assert not bad, f"{len(bad)} cases differ from their reference under poison; the first: {bad[:10]}"
    assert not res["dirty"], f"{len(res['dirty'])} scratch checks came back dirty; the first: {res['dirty'][:5]}"
    here = {}
    for family in sw.FAMILIES:
        here.update({_key(r): r["sha256"] for r in _family(ctx, family)["records"]})
    there = {_key(r): r["sha256"] for r in res["records"]}
    poison_child.assert_unmoved(here, there)
