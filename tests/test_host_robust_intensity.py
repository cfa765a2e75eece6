"""Robust per-cell intensity statistics (AMT_RPX_ROBUST), the parts that need no device: the numpy reference against a
sort-and-index restatement and hand-worked rows, the header's and the binding's constants, the key names, the rank rule
of csrc/amt_rank_rule.h built with the host compiler against np.percentile, and what the case list holds."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import robust_cases as qc
import robust_reference as qr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "arcadia_microscopy_tools_amd", "csrc")


def _header():
    with open(os.path.join(ROOT, "include", "amt_hip.h")) as f:
        return f.read()


def _define(header, name):
    m = re.search(r"#define\s+" + name + r"\s+(\S+.*)", header)
    assert m, name
    return m.group(1).strip()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def test_reference_hand_worked_rows():
    assert qr.robust_row([1, 2, 3, 4]).tolist() == [1.75, 2.5, 3.25, 1.0]
    assert qr.robust_row(np.array([7], np.uint16)).tolist() == [7.0, 7.0, 7.0, 0.0]
    assert qr.robust_row(np.array([0, 65535], np.uint16)).tolist() == [16383.75, 32767.5, 49151.25, 32767.5]
    assert qr.robust_row([1, 2, 3]).tolist() == [1.5, 2.0, 2.5, 1.0]
    assert qr.robust_row([5, 1, 100, 3, 2]).tolist() == [2.0, 3.0, 5.0, 2.0]  # one outlier moves neither median nor MAD
    assert qr.robust_row(np.array([0, 65535] * 3, np.uint16)).tolist() == [0.0, 32767.5, 65535.0, 32767.5]
    assert np.isnan(qr.robust_row(np.zeros(0, np.uint16))).all()
    lab = np.array([[1, 1, 0, 3], [1, 1, 3, 3]])
    img = np.array([[1, 2, 9, 10], [3, 4, 20, 30]], np.uint16)
    got = qr.robust_columns(lab, img, 4)
    assert got[0].tolist() == [1.75, 2.5, 3.25, 1.0] and got[2].tolist() == [15.0, 20.0, 25.0, 10.0]
    assert np.isnan(got[1]).all() and np.isnan(got[3]).all()
    assert qr.robust_stack(lab, np.stack([img, img]), 4).shape == (4, 2, 4)


def test_reference_equals_sort_and_index():
    rng = np.random.RandomState(5)
    for i in range(400):
        n = rng.randint(1, 70)
        for v in (rng.randint(0, 65536, n).astype(np.uint16), rng.randint(0, 4, n).astype(np.uint16),
                  rng.normal(0, 1e3, n), rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-300, 300, n)):
            assert _bits(qr.robust_row(v)) == _bits(qr.sort_and_index_row(v)), (i, v)


def test_header_defines_and_documents_the_statistics():
    h = _header()
    assert eval(_define(h, "AMT_RPX_ROBUST").replace("u", "")) == 512
    assert _define(h, "AMT_RPX_ALL") == "0xffu"
    assert eval(_define(h, "AMT_RPX_RELATE").replace("u", "")) == 256
    assert [int(_define(h, "AMT_RPX_QCOL_" + n)) for n in ("Q25", "MEDIAN", "Q75", "MAD")] == [0, 1, 2, 3]
    B = int(_define(h, "AMT_ROBUST_LDS_BINS"))
    assert B >= 1024 and B & (B - 1) == 0
    # the new defines follow AMT_RELATE_LDS_PARTNERS, the new block stands before the relate block
    assert h.index("#define AMT_RELATE_LDS_PARTNERS") < h.index("#define AMT_RPX_ROBUST") < h.index("#define AMT_RPX_COL_EULER")
    assert h.index("AMT_RPX_ROBUST ----") < h.index("AMT_RPX_RELATE ----")
    block = h[h.index("AMT_RPX_ROBUST ----"):h.index("AMT_RPX_RELATE ----")]
    for word in ("np.percentile", "linear", "AMT_RPX_QCOL_Q25", "AMT_RPX_QCOL_MEDIAN", "AMT_RPX_QCOL_Q75",
                 "AMT_RPX_QCOL_MAD", "1.4826", "np.median", "AMT_U16", "AMT_F64", "NaN", "infinities", "AMT_EINVAL",
                 "AMT_RPX_CENTROID_WEIGHTED", "AMT_RPX_RELATE", "AMT_ROBUST_LDS_BINS", "identical bytes",
                 "AMT_RPX_ALL | AMT_RPX_RELATE | AMT_RPX_ROBUST", "before the first launch"):
        assert word in block, word


def test_binding_constants_equal_the_header():
    from arcadia_microscopy_tools_amd import _hip

    h = _header()
    assert _hip.RPX_ROBUST == 512 == 1 << 9
    assert _hip.RPX_QCOLS == ("q25", "median", "q75", "mad") == qr.COLS
    assert _hip.ROBUST_LDS_BINS == int(_define(h, "AMT_ROBUST_LDS_BINS"))
    with open(os.path.join(CSRC, "amt_robust.hip")) as f:
        src = f.read()
    assert re.search(r"RB_BINS\s*=\s*AMT_ROBUST_LDS_BINS\s*;", src)  # the kernel's table is sized by that name
    assert re.search(r"__shared__\s+unsigned\s+tab\[RB_BINS\]", src)
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert "amt_robust.hip" in f.read()


def test_existing_names_are_unchanged():
    from arcadia_microscopy_tools_amd import _hip

    assert _hip.RPX_BITS == {
        "euler_number": 1, "perimeter_crofton": 2, "area_filled": 4, "feret_diameter_max": 8, "centroid_local": 16,
        "inertia_tensor": 32, "inertia_tensor_eigvals": 64, "centroid_weighted": 128, "centroid_weighted_local": 128}
    assert _hip.RPX_COLS == (
        "euler_number", "perimeter_crofton", "area_filled", "feret_diameter_max", "centroid_local-0", "centroid_local-1",
        "inertia_tensor-0-0", "inertia_tensor-0-1", "inertia_tensor-1-0", "inertia_tensor-1-1",
        "inertia_tensor_eigvals-0", "inertia_tensor_eigvals-1")
    assert _hip.RPX_WCOLS == ("centroid_weighted-0", "centroid_weighted-1", "centroid_weighted_local-0",
                              "centroid_weighted_local-1")
    assert _hip.RPX_RCOLS == ("parent", "overlap", "partners", "area") and _hip.RPX_RELATE == 256
    # the capability rides on amt_regionprops_ext: no entry point of its own
    assert "amt_regionprops_ext" in _hip._SIGS
    assert not [name for name in _hip._SIGS if "robust" in name or "quantile" in name or "mad" in name.split("_")]
    protos = set(re.findall(r"^int\s+(amt_\w+)\s*\(", _header(), flags=re.M))
    assert not [name for name in protos if "robust" in name]


def test_robust_intensity_keys():
    from arcadia_microscopy_tools_amd import segment
    from arcadia_microscopy_tools_amd.channels import DAPI, FITC

    assert segment.robust_intensity_keys(["DAPI"]) == ["intensity_q25_dapi", "intensity_median_dapi",
                                                       "intensity_q75_dapi", "intensity_mad_dapi"]
    keys = segment.robust_intensity_keys([FITC, DAPI])
    assert keys == [f"intensity_{s}_{c}" for c in ("fitc", "dapi") for s in ("q25", "median", "q75", "mad")]
    assert segment.robust_intensity_keys([]) == []
    # cell_properties keeps its names: none of the new ones is accepted or produced there
    assert not [k for k in segment.cell_property_keys(["DAPI"]) if "median" in k or "q25" in k or "mad" in k]


PROGRAM = r"""
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "amt_rank_rule.h"

static void put(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    std::printf(" %016llx", (unsigned long long)u);
}

// input: records "kind n v0 .. v(n-1)" of ascending values; kind 0 = uint16 in decimal, 1 = float64 as hex bit patterns
int main() {
    int kind;
    unsigned long long n;
    while (std::scanf("%d %llu", &kind, &n) == 2) {
        if (kind == 0) {
            std::vector<unsigned> v(n);
            for (auto& x : v) if (std::scanf("%u", &x) != 1) return 2;
            amt_rank r[3];
            for (int q = 0; q < 3; ++q) {
                r[q] = amt_rank_of(n, 0.25 * (q + 1));
                if (r[q].hi >= n || r[q].lo > r[q].hi) return 3;
                // the integer form and the float64 lerp give the same bits
                const double a = amt_quartile_u16(v[r[q].lo], v[r[q].hi], amt_rank_quarters(r[q].t));
                if (a != amt_np_lerp((double)v[r[q].lo], (double)v[r[q].hi], r[q].t)) return 4;
                put(a);
            }
            const bool odd = n & 1;
            const unsigned m2 = amt_median2_u16(v[r[1].lo], v[r[1].hi], odd);
            std::vector<unsigned> k(n);
            for (size_t i = 0; i < n; ++i) k[i] = 2 * v[i] > m2 ? 2 * v[i] - m2 : m2 - 2 * v[i];
            std::sort(k.begin(), k.end());
            put(amt_mad_u16(k[r[1].lo], k[r[1].hi], odd));
        } else {
            std::vector<double> v(n);
            for (auto& x : v) {
                unsigned long long u;
                if (std::scanf("%llx", &u) != 1) return 2;
                std::memcpy(&x, &u, 8);
            }
            amt_rank r[3];
            double res[3];
            for (int q = 0; q < 3; ++q) {
                r[q] = amt_rank_of(n, 0.25 * (q + 1));
                if (r[q].hi >= n || r[q].lo > r[q].hi) return 3;
                res[q] = amt_np_lerp(v[r[q].lo], v[r[q].hi], r[q].t);
                put(res[q]);
            }
            std::vector<double> d(n);
            for (size_t i = 0; i < n; ++i) d[i] = std::fabs(v[i] - res[1]);
            std::sort(d.begin(), d.end());
            put(amt_np_lerp(d[r[1].lo], d[r[1].hi], r[1].t));
        }
        std::printf("\n");
    }
    return 0;
}
"""


def test_rank_rule_header_equals_numpy(tmp_path):
    """amt_rank_rule.h has no HIP include: built with the host compiler, its ranks, lerp and integer forms give
    np.percentile's bits for every count from 1 to 300."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler found (g++ / c++ / clang++)")
    src = tmp_path / "rule.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "rule"
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", "-O1", "-ffp-contract=off", "-I", CSRC, "-o", str(exe),
                           str(src)])
    rng = np.random.RandomState(11)
    lines, want = [], []
    for n in range(1, 301):
        u = np.sort(rng.randint(0, 65536 if n % 3 else 5, n).astype(np.uint16))
        lines.append("0 %d %s" % (n, " ".join(str(int(x)) for x in u)))
        want.append(qr.robust_row(u))
        f = np.sort(rng.normal(0.0, 1e3, n) if n % 2 else rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-300, 300, n))
        lines.append("1 %d %s" % (n, " ".join("%016x" % x for x in f.view(np.uint64))))
        want.append(qr.robust_row(f))
    run = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr)
    rows = run.stdout.strip().split("\n")
    assert len(rows) == len(want) == 600
    for i, (row, w) in enumerate(zip(rows, want)):
        got = np.array([int(x, 16) for x in row.split()], np.uint64).view(np.float64)
        assert got.tobytes() == w.tobytes(), (i // 2 + 1, "u16" if i % 2 == 0 else "f64", got, w)


def test_the_cases_hold_what_they_are_named_for():
    B = qc._bins()
    for shape in qc.SHAPES:
        for kind in qc.KINDS:
            cs = qc.cases(shape, kind)
            assert {"blobs", "gaps", "pieces", "small_counts", "column_and_row", "constants", "channels_2", "channels_3",
                    "channels_5"} <= set(cs)
            for name, (lab, stack, k) in cs.items():
                assert lab.dtype == np.int32 and lab.shape == shape and stack.dtype == qc.DTYPE[kind], name
                assert stack.ndim == 3 and stack.shape[1:] == shape and k >= 1, name
                assert np.isfinite(stack).all(), name
            assert [cs[f"channels_{C}"][1].shape[0] for C in (2, 3, 5)] == [2, 3, 5]
            # the constants: a constant label, all lowest, all highest, all equal but one, half / half
            ref = qc.reference(shape, kind, "constants")[:, 0]
            lo, hi = (0.0, 65535.0) if kind == "u16" else (0.0, 1e300)
            assert ref[0, 0] == ref[0, 2] and ref[0, 3] == 0 and ref[1].tolist() == [lo] * 3 + [0.0]
            assert ref[2].tolist() == [hi] * 3 + [0.0] and ref[3, 1] == ref[0, 1] and ref[3, 3] == 0
            if kind == "u16":
                assert ref[4, 1] == 32767.5 and ref[4, 3] == 32767.5
            gaps = qc.reference(shape, kind, "gaps")[:, 0]
            assert np.isnan(gaps[1::3]).all() and np.isnan(gaps[-2:]).all() and np.isfinite(gaps[2::3]).any()
            # label 1 lies in pieces among extreme values of other labels that must not count
            lab, stack, _ = cs["pieces"]
            inside = stack[0][lab == 1]
            y, x = np.nonzero(lab == 1)
            box = stack[0][y.min():y.max() + 1, x.min():x.max() + 1]
            assert box.max() > inside.max() * 10 and box.min() < inside.min()
    counts = np.bincount(qc.cases((33, 40), "u16")["small_counts"][0].ravel())[1:]
    assert counts.tolist() == [1, 2, 3, 4, 5, 6, 7, 8]
    assert np.bincount(qc.cases((7, 5), "f64")["small_counts"][0].ravel())[1:].tolist() == [1, 2, 3, 4, 5, 6, 7]
    lab = qc.cases((70, 131), "u16")["column_and_row"][0]
    assert (lab == 2).any(axis=0).sum() > 64 and (lab == 1).any(axis=0).sum() == 1
    lab, stack, k = qc.cases(qc.BIG, "u16")["one_label"]
    assert k == 1 and (lab == 1).sum() == 67600 > 65535
    for shape in qc.SHAPES:
        cs = qc.cases(shape, "u16")
        W = shape[1]
        for name, levels in qc._levels(B).items():
            v = cs[f"levels_{name}"][1][0].ravel()[W:].astype(np.int64)
            assert v.max() - v.min() + 1 == levels, (shape, name)
        step = 65536 // B
        lab, stack, _ = cs["ranks_one_bin"]
        v = np.sort(stack[0][lab == 1].astype(np.int64))
        n = len(v)
        assert v[0] == 0 and v[-1] == 65535
        ranks = sorted({int(np.floor((n - 1) * q)) + d for q in (0.25, 0.5, 0.75) for d in (0, 1)})
        assert len({int(v[r]) // step for r in ranks}) == 1
        v = np.sort(cs["ranks_three_bins"][1][0][cs["ranks_three_bins"][0] == 1].astype(np.int64))
        n = len(v)
        assert v[-1] - v[0] >= 2 * B
        if n >= 20:
            assert len({int(v[int(np.floor((n - 1) * q))] - v[0]) // step for q in (0.25, 0.5, 0.75)}) == 3
        lab, stack, _ = cs["rank_straddle"]
        v = np.sort(stack[0][lab == 1].astype(np.int64))
        n = len(v)
        assert n % 2 == 0 and v[0] == 0 and v[-1] == 65535 and v[n // 2 - 1] // step != v[n // 2] // step
        lab, stack, _ = cs["mad_keys_wide"]
        v = stack[0][lab == 1].astype(np.int64)
        med2 = int(round(2 * np.percentile(v, 50)))
        assert v.max() - v.min() < B <= np.abs(2 * v - med2).max()
    # float64: one sign of zero per label where a rank can land on it, both where none can; subnormals; magnitudes
    lab, stack, _ = qc.cases((33, 40), "f64")["float_specials"]
    v = [stack[0][lab == l] for l in range(1, 7)]
    assert np.signbit(v[0][v[0] == 0]).all() and (v[0] == 0).any() and (v[0] < 0).any()
    assert not np.signbit(v[1][v[1] == 0]).any() and (v[1] == 0).any()
    z = v[2][v[2] == 0]
    assert len(z) == 2 and np.signbit(z).tolist() == [True, False] and (len(v[2]) - 1) // 4 >= 2
    assert (np.abs(v[3]) < 2.3e-308).all() and (v[3] != 0).all()
    assert np.log10(np.abs(v[4]).max()) - np.log10(np.abs(v[4]).min()) > 300 and (v[4] < 0).any()
    assert len(np.unique(v[5])) <= 4
