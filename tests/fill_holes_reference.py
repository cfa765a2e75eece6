"""Test-side reference for ``binary_fill_holes`` (not collected): scipy's answer, the component restatement the device
implements, and seeded generators of planes whose result is known by construction.

The rule: ``out[p] = in[p] != 0``, or p lies in a component of the background that holds no pixel of the 1-pixel frame
(row 0, row H-1, column 0, column W-1); background components are 4-connected for the 3 x 3 cross and 8-connected for the
3 x 3 all-ones structure.  scipy reaches the background by propagating from outside the image, which is the same thing
for exactly these two structures (tests/test_host_fill_holes.py checks it on every shape below).

Every generator returns a uint8 0 / 1 plane of the asked shape, or None where the shape is too small for what it builds;
its stated property is checked against scipy by the host test.
"""
from __future__ import annotations

import numpy as np
from scipy import ndimage as ndi

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], np.uint8)
FULL = np.ones((3, 3), np.uint8)
STRUCTURES = (("cross", CROSS), ("full", FULL))

# the operator sweep's shapes (without its second 256-wide Gaussian shape), the smallest plane that can hold a hole
# (3, 3), and one plane of 256 x 256: 16 tiles, for the spiral
SHAPES = [(1, 1), (1, 17), (19, 1), (2, 2), (3, 3), (7, 5), (16, 16), (15, 24), (17, 32), (33, 40), (64, 64), (65, 128),
          (70, 131), (9, 256), (40, 256), (66, 320), (256, 256)]
SPIRAL_SHAPES = [(7, 5), (16, 16), (33, 40), (65, 128), (70, 131), (66, 320), (256, 256)]
SEEDS = (0, 1, 2)
DENSITIES = (0.5, 0.65, 0.8)  # of the random planes, one per seed


def scipy_fill(mask, structure) -> np.ndarray:
    """scipy's answer as uint8 0 / 1."""
    m = np.asarray(mask) != 0
    if m.size == 0:
        return np.zeros(m.shape, np.uint8)
    return ndi.binary_fill_holes(m, structure=np.asarray(structure) != 0).astype(np.uint8)


def component_fill(mask, structure) -> np.ndarray:
    """The restatement: background components (connectivity of ``structure``) without a frame pixel are filled."""
    m = np.asarray(mask) != 0
    lab, k = ndi.label(~m, structure=np.asarray(structure) != 0)
    frame = np.zeros(m.shape, bool)
    frame[0, :] = frame[-1, :] = True
    frame[:, 0] = frame[:, -1] = True
    touching = np.unique(lab[frame])
    holes = np.setdiff1d(np.arange(1, k + 1), touching)
    return (m | np.isin(lab, holes)).astype(np.uint8)


# ---- generators -----------------------------------------------------------------------------------------------------
def random(shape, density, seed):
    """Independent pixels, foreground with probability ``density``."""
    rng = np.random.default_rng([seed, shape[0], shape[1], int(density * 1000)])
    return (rng.random(shape) < density).astype(np.uint8)


def all_zero(shape):
    return np.zeros(shape, np.uint8)


def all_one(shape):
    return np.ones(shape, np.uint8)


def frame_only(shape):
    """A 1-pixel ring on the frame: the result is all ones (for H, W >= 3 the interior is one hole)."""
    m = np.zeros(shape, np.uint8)
    m[0, :] = m[-1, :] = 1
    m[:, 0] = m[:, -1] = 1
    return m


def checkerboard(shape):
    """Foreground where y + x is even: under the cross every interior background pixel is a hole of its own, under
    all-ones the background is one component that reaches the frame.  The complement's worst case for runs: 32 per
    64-pixel row."""
    y, x = np.indices(shape)
    return ((y + x) % 2 == 0).astype(np.uint8)


def stripes_1px(shape):
    """Vertical 1-pixel stripes (odd columns are foreground): every background column reaches row 0, nothing is filled."""
    m = np.zeros(shape, np.uint8)
    m[:, 1::2] = 1
    return m


def spiral(shape, open=True):
    """A solid plane into which a 1-pixel background corridor is carved: from a mouth on the frame at (1, 0) it winds
    clockwise to the centre, a 1-pixel wall between its turns.  ``open``: the mouth is background and nothing is filled;
    closed (the mouth pixel set): the whole corridor is one hole and the result is all ones."""
    H, W = shape
    if H < 5 or W < 5:
        return None
    m = np.ones(shape, np.uint8)
    y, x, dy, dx = 1, 0, 0, 1
    m[y, x] = 0

    def can_step(y, x, dy, dx):
        ny, nx = y + dy, x + dx
        if not (1 <= ny <= H - 2 and 1 <= nx <= W - 2) or not m[ny, nx]:
            return False
        ay, ax = ny + dy, nx + dx  # the cell behind it must stay a wall
        return bool(m[ay, ax])

    while True:
        if can_step(y, x, dy, dx):
            y, x = y + dy, x + dx
            m[y, x] = 0
            continue
        dy, dx = dx, -dy  # turn right
        if not can_step(y, x, dy, dx):
            break
    if not open:
        m[1, 0] = 1
    return m


def nested(shape):
    """A block with a hole that holds an island that holds a hole: the result is the solid block."""
    H, W = shape
    if H < 9 or W < 9:
        return None
    m = np.zeros(shape, np.uint8)
    m[1:-1, 1:-1] = 1
    m[2:-2, 2:-2] = 0
    m[3:-3, 3:-3] = 1
    m[4:-4, 4:-4] = 0
    return m


def nested_solid(shape):
    m = np.zeros(shape, np.uint8)
    m[1:-1, 1:-1] = 1
    return m


def diagonal_leak(shape):
    """Solid but for the pixels (i, i), i = 0 .. min(H, W) // 2: background joined to the corner only by diagonal steps.
    Filled under the cross (but for the corner itself), left alone under all-ones."""
    H, W = shape
    if H < 3 or W < 3:
        return None
    m = np.ones(shape, np.uint8)
    for i in range(min(H, W) // 2 + 1):
        m[i, i] = 0
    return m


def corner_touch(shape):
    """Solid but for the bottom-right corner and two pixels diagonally inside it: under all-ones a background component
    whose only frame pixel is a corner (kept), under the cross the corner alone (kept) and a 2-pixel hole (filled)."""
    H, W = shape
    if H < 3 or W < 4:
        return None
    m = np.ones(shape, np.uint8)
    m[H - 1, W - 1] = 0
    m[H - 2, W - 2] = 0
    m[H - 2, W - 3] = 0
    return m


def row1_hole(shape):
    """Solid but for the four pixels diagonally inside the corners: holes in row 1 / column 1 (and row H-2 / column
    W-2) that do not touch the frame.  The result is all ones."""
    H, W = shape
    if H < 3 or W < 3:
        return None
    m = np.ones(shape, np.uint8)
    m[1, 1] = m[1, W - 2] = m[H - 2, 1] = m[H - 2, W - 2] = 0
    return m


def seam_bay(shape):
    """The only background ``seam_holes`` leaves after filling: a 1-pixel bay from row 0."""
    m = np.ones(shape, np.uint8)
    m[0:3, shape[1] // 2] = 0
    return m


def seam_holes(shape):
    """Solid, with holes that straddle columns 63|64 and rows 63|64 (where the plane has them), a hole in the last
    pixels before the right frame column (the ragged last word of width 131), and a bay open to row 0 that must stay."""
    H, W = shape
    if H < 5 or W < 6:
        return None
    m = seam_bay(shape)
    if W >= 67:
        m[H - 3:H - 1, 62:66] = 0
    if H >= 67:
        m[62:66, 1:3] = 0
    if H >= 67 and W >= 67:
        m[63, 63] = m[64, 64] = 0  # where four tiles meet: two holes under the cross, one under all-ones
    m[H // 2, W - 4:W - 1] = 0
    return m


def truth_bytes(plane, seed):
    """The same plane with its foreground bytes drawn from {1, 2, 255}."""
    rng = np.random.default_rng([seed, plane.shape[0], plane.shape[1]])
    vals = rng.choice(np.array([1, 2, 255], np.uint8), size=plane.shape)
    return np.where(plane != 0, vals, 0).astype(np.uint8)


def planes(shape):
    """[(name, plane)] of every generator that fits ``shape``."""
    out = [(f"random-{s}", random(shape, DENSITIES[i], s)) for i, s in enumerate(SEEDS)]
    out += [("all_zero", all_zero(shape)), ("all_one", all_one(shape)), ("frame_only", frame_only(shape)),
            ("checkerboard", checkerboard(shape)), ("stripes_1px", stripes_1px(shape))]
    if shape in SPIRAL_SHAPES:
        out += [("spiral-open", spiral(shape, True)), ("spiral-closed", spiral(shape, False))]
    out += [("nested", nested(shape)), ("diagonal_leak", diagonal_leak(shape)), ("corner_touch", corner_touch(shape)),
            ("row1_hole", row1_hole(shape)), ("seam_holes", seam_holes(shape))]
    return [(n, p) for n, p in out if p is not None]


def annuli_field(size=256, count=12, seed=11):
    """A four-channel uint16 field whose DAPI channel (index 1) is ``count`` annuli on a dim background: outer radius
    14-18, wall 5, so the rings survive Otsu and a closing with disk(2) cannot bridge their centres."""
    rng = np.random.default_rng(seed)
    y, x = np.indices((size, size))
    dapi = np.full((size, size), 300.0)
    centres = []
    tries = 0
    while len(centres) < count and tries < 10000:
        tries += 1
        r = int(rng.integers(14, 19))
        cy, cx = rng.integers(r + 3, size - r - 3, 2)
        if all((cy - a) ** 2 + (cx - b) ** 2 > (r + c + 4) ** 2 for a, b, c in centres):
            centres.append((int(cy), int(cx), r))
    for cy, cx, r in centres:
        d = np.hypot(y - cy, x - cx)
        dapi[(d <= r) & (d >= r - 5)] = 9000.0
    dapi += rng.normal(0, 40, dapi.shape)
    fov = np.empty((4, size, size), np.uint16)
    for c in range(4):
        fov[c] = np.clip(rng.normal(500, 50, (size, size)), 0, 65535).astype(np.uint16)
    fov[1] = np.clip(dapi, 0, 65535).astype(np.uint16)
    return fov, centres
