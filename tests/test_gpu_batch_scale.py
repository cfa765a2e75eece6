"""The work-size table (tests/batch_scale_cases.py) on the device: every group against its references with every plane of
every batch compared, the variant the model says each call took in the report, and the whole table once more in a child
process under AMT_DEBUG_POISON=1 -- no mismatch, no stray write behind a scratch buffer, every output digest equal to the
in-process run's."""
import numpy as np
import pytest

import batch_scale_cases as bs
import poison_child

pytestmark = pytest.mark.gpu

# the child's time limit: ten times the in-process run of the table on an MI355X, rounded up to a whole minute
# (profiles/batch_scale.json: 14.6 s measured, references included)
CHILD_TIMEOUT_S = 180

_RESULTS: dict = {}


@pytest.fixture(scope="module")
def ctx():
    from arcadia_microscopy_tools_amd.device import get_context

    return get_context()


def _group(ctx, group):
    """The in-process run of one group: made once, shared with the poison test."""
    if group not in _RESULTS:
        _RESULTS[group] = bs.run(ctx, [group])
    return _RESULTS[group]


def _mismatches(records):
    return [(r["group"], r["op"], r["param"], tuple(r["shape"]), r["nplanes"], r["variant"], r["index"])
            for r in records if r["status"] != "pass"]


def _key(r):
    return (r["group"], r["op"], r["param"], tuple(r["shape"]), r["nplanes"])


@pytest.mark.parametrize("group", bs.GROUPS)
def test_group_matches_its_references(ctx, group):
    num_cus = bs.num_cus_of(ctx.device_name())
    for case in bs.table(group):  # a clear message before anything runs, should this chip not reach a side
        bs.check_reach(case, num_cus)
    res = _group(ctx, group)
    assert len(res["records"]) == len(bs.table(group))
    print(f"\n{group} ({num_cus} CUs, {res['seconds']:.1f} s):")
    for variant, calls in bs.variants_of(res["records"])[group].items():
        print(f"  {calls:4d} x {variant}")
    bad = _mismatches(res["records"])
    assert not bad, f"{len(bad)} of {len(res['records'])} calls differ from their reference; the first: {bad[:10]}"
    # the sides the group is there for were both taken
    sides = {c.switch: set() for c in bs.table(group) if c.switch}
    for c in bs.table(group):
        if c.switch:
            sides[c.switch].add(c.side)
    assert all(v == {"far", "near"} for v in sides.values()), sides


def test_d2_does_not_depend_on_the_tile_variant(ctx):
    """The same batch through edt_bits_kernel<64, 16> (d2 alone) and <32, 24> (both outputs): identical d2."""
    from arcadia_microscopy_tools_amd import hipops

    recs = {(tuple(r["shape"]), r["param"]): r for r in _group(ctx, "edt tile variant")["records"]}
    lim = bs.limits()
    for shape in bs.EDT_SHAPES:
        n = bs.first_far(lambda k: bs.edt_tiles(shape, k) >= lim["EDT_TILES"])
        order = bs.layout(n, len(bs.EDT_SLOTS))
        mask = ctx.asarray(np.stack([bs.edt_plane(shape, bs.EDT_SLOTS[s]) for s in order]))
        alone = hipops.edt(mask, want_edt=False)[0].numpy()
        both = hipops.edt(mask)[0].numpy()
        assert np.array_equal(alone, both), (shape, np.argwhere(alone != both)[0])
        assert any(k[0] == shape and "d2 alone" in k[1] and "<64, 16>" in r["variant"] for k, r in recs.items())
        assert any(k[0] == shape and "d2 and edt" in k[1] and "<32, 24>" in r["variant"] for k, r in recs.items())


def test_table_under_poison(ctx, tmp_path):
    out = tmp_path / "batch_scale.json"
    res = poison_child.run_module("tests.batch_scale_cases", out, CHILD_TIMEOUT_S, "the poisoned table")
    bad = _mismatches(res["records"])
    assert not bad, f"{len(bad)} calls differ from their reference under poison; the first: {bad[:10]}"
    assert not res["dirty"], f"{len(res['dirty'])} scratch checks came back dirty; the first: {res['dirty'][:5]}"
    here = {}
    for group in bs.GROUPS:
        here.update({_key(r): r["sha256"] for r in _group(ctx, group)["records"]})
    there = {_key(r): r["sha256"] for r in res["records"]}
    poison_child.assert_unmoved(here, there)
