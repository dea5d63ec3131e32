"""The rows of tests/test_gpu_ssim_plan.py, the launch plan of the SSIM kernels written out a second time, the inputs that make
the plan's seams visible in a score, and SSIM as a map in plain float64 NumPy.  No GPU and no library of the project is used
here: tests/test_ssim_plan_cpu.py holds ``plan`` against csrc/ke_ssim_plan.h, tests/test_ssim_plan_cases_cpu.py holds the inputs
to the visibility condition, and the GPU test holds the kernels to the oracle on them.

The plan (``plan``; the rules, nothing of it read from the header).  One wave scores one (pair, block of columns, band of
rows).  A lane owns px = 4 or 8 columns, a wave 64 px columns of which 64 px - 6 are interior ones: 250 or 506.  px is 8 where
ceil((w-6)/506) * 506 < ceil((w-6)/250) * 250, else 4.  Rows are read as whole dwords (aligned) where the width is a multiple of 4
(else why = WIDTH), the base address and the image's bytes are multiples of 4 (else why = BASE) and there is one block, or blocks
of 248 / 504 columns do not add a block (else why = BLOCKS); aligned blocks of several are 248 / 504 columns wide.  A side under 7:
NaN fill.  Fewer than 4096 windows, or exact mode: the exact kernel, bands of 64 rows.  Else the fast kernel: with g = ceil((h-6)/7)
groups of seven rows, G = g * pairs * blocks // 8192 kept within 2..18, then G = ceil(g / ceil(g / G)), at least 2; bands of 7 G rows.

The inputs (``pixels``).  Image a is seeded noise, 128 plus or minus 32..48, so that every pixel carries about the same share of a
window's variance.  Image b is 128 + g (a - 128): g = 1 (b is a) at strength 0, g = 0.27 at strength 1 and g = 0 (flat) at strength
2 -- or, where a picture has only two strengths, 1 and 0.  The strength of a pixel is one step for the seams of the plan to its
left, taken modulo 2, and one for the seams above it, modulo 2.  A block seam lies at map column k * block_cols, pixel column + 3;
a band seam at map row k * band_rows, pixel row + 3, for the bands of both kernels.  The covariance of a window is g times the
variance of a, so S is about 1, 0.5 and 0.04 at the three strengths and changes by a seventh of a step per map column or row
across every seam, in the same direction in every row (column) of it and without changing sign: a window dropped, doubled or
taken from the neighbouring lane or row there moves the mean.  (Independent noise switched on and off would step up in one band and
down in the next, so that the two errors cancel in the mean, and the step from one window to the next would be smaller than its
own scatter.)  The family "lanes" takes its steps every px columns and every 7 rows instead, the first after 4 columns and after 4 rows, for
the lane seams inside a block and the picture's edges: the widths of its rows are such that the last two windows of a row of the
map do not hold equally many columns of either strength."""
from __future__ import annotations

import zlib

import numpy as np

NAN, EXACT, FAST = 0, 1, 2                                   # entry [0] of ke_last_ssim_plan
TAKEN, WIDTH, BASE, BLOCKS = 0, 1, 2, 3                      # entry [7]
KERNEL, PX, ALIGNED, COL_BLOCKS, BLOCK_COLS, BAND_ROWS, BANDS, WHY = range(8)
BAR = {EXACT: 1e-6, FAST: 1e-5}                              # the bars of tests/test_gpu_parity.py


def plan(w, h, channels, pairs, base_mod4, exact_mode):
    """The plan of a launch as a dict; w may be an array (the others scalars), then every entry is one."""
    small = (np.asarray(w, np.int64) < 7) | (h < 7)
    w, h = np.maximum(np.asarray(w, np.int64), 7), max(h, 7)              # (a side under 7 is planned as 7 and blanked below)
    ceil = lambda a, b: -(-a // b)
    cb4, cb8 = ceil(w - 6, 250), ceil(w - 6, 506)
    px = np.where(cb8 * 506 < cb4 * 250, 8, 4)
    blocks = np.where(px == 8, cb8, cb4)
    why = np.where(w % 4 != 0, WIDTH, np.where((base_mod4 % 4 != 0) | (w * h * channels % 4 != 0), BASE, TAKEN))
    narrow = 64 * px - 8                                     # 248 or 504
    why = np.where((why == TAKEN) & (blocks > 1) & (ceil(w - 6, narrow) != blocks), BLOCKS, why)
    cols = np.where((why == TAKEN) & (blocks > 1), narrow, 64 * px - 6)
    exact = np.full(w.shape, bool(exact_mode)) | ((w - 6) * (h - 6) < 4096)
    groups = ceil(h - 6, 7)
    G = np.clip(groups * pairs * blocks // 8192, 2, 18)
    G = np.maximum(ceil(groups, ceil(groups, G)), 2)
    band_rows = np.where(exact, 64, 7 * G)
    bands = ceil(h - 6, band_rows)
    p = dict(kernel=np.where(exact, EXACT, FAST), px=px, aligned=(why == TAKEN).astype(np.int64), col_blocks=blocks, block_cols=cols,
             band_rows=band_rows, bands=bands, items_per_pair=blocks * bands, n_items=pairs * blocks * bands, why=why)
    p = {k: np.where(small, NAN if k == "kernel" else -1, v) for k, v in p.items()}
    return p if w.ndim else {k: int(v) for k, v in p.items()}


def words(p: dict) -> tuple:
    """A plan as ke_last_ssim_plan reports it."""
    return (p["kernel"], p["px"], p["aligned"], p["col_blocks"], p["block_cols"], p["band_rows"], p["bands"], p["why"])


class Row:
    """One launch shape and the branch it is there for.  `exact`: the mode the branch was worked out for (every row is scored in
    both).  `base`: 0 for images handed over from the host, else the images lie in device memory `base` bytes past an
    allocation's start.  `distinct`: image pairs the launch cycles through.  `want`: entries of the plan the row must show."""

    def __init__(self, name, w, h, channels, exact, *, pairs=1, base=0, family="seams", distinct=1, **want):
        self.name, self.w, self.h, self.channels, self.exact, self.pairs, self.base = name, w, h, channels, exact, pairs, base
        self.family, self.distinct, self.want = family, distinct, want

    def plan(self, exact_mode: bool) -> dict:
        return plan(self.w, self.h, self.channels, self.pairs, self.base, exact_mode)


def _grid() -> list:
    """Every (kernel, channels, px, aligned, one or several blocks): the exact kernel on one row of windows (N = w - 6, so one
    wrong window is worth 1e-3 against 1e-6), the fast one at the smallest height with 4096 windows."""
    shapes = [  # width, height of the fast row, px, aligned, blocks, block_cols, why
        (64, 90, 4, 1, 1, 250, TAKEN), (63, 78, 4, 0, 1, 250, WIDTH), (760, 12, 4, 1, 4, 248, TAKEN), (504, 15, 4, 0, 2, 250, BLOCKS),
        (512, 15, 8, 1, 1, 506, TAKEN), (509, 15, 8, 0, 1, 506, WIDTH), (1012, 11, 8, 1, 2, 504, TAKEN), (1010, 11, 8, 0, 2, 506, WIDTH),
    ]
    rows = []
    for w, hf, px, al, blocks, cols, why in shapes:
        for ch in (1, 3, 4):
            want = dict(px=px, aligned=al, col_blocks=blocks, block_cols=cols, why=why)
            rows.append(Row(f"exact_{w}x7_c{ch}", w, 7, ch, True, kernel=EXACT, band_rows=64, bands=1, **want))
            rows.append(Row(f"fast_{w}x{hf}_c{ch}", w, hf, ch, False, kernel=FAST, band_rows=14, **want))
    return rows


ROWS = _grid() + [
    # the widths whose aligned data goes to the funnel-shift loader, because blocks of 248 / 504 columns would add one
    Row("exact_756x7_blocks", 756, 7, 1, True, kernel=EXACT, px=4, aligned=0, col_blocks=3, block_cols=250, why=BLOCKS),
    Row("fast_756x12_blocks", 756, 12, 3, False, kernel=FAST, px=4, aligned=0, col_blocks=3, why=BLOCKS),
    Row("exact_1016x7_blocks", 1016, 7, 3, True, kernel=EXACT, px=8, aligned=0, col_blocks=2, block_cols=506, why=BLOCKS),
    Row("fast_1016x11_blocks", 1016, 11, 1, False, kernel=FAST, px=8, aligned=0, col_blocks=2, why=BLOCKS),
    Row("exact_1520x7_blocks", 1520, 7, 4, True, kernel=EXACT, px=8, aligned=0, col_blocks=3, why=BLOCKS),
    Row("fast_1520x9_blocks", 1520, 9, 1, False, kernel=FAST, px=8, aligned=0, col_blocks=3, why=BLOCKS),
    # three aligned blocks of 504, and of 1012 + 4
    Row("exact_1512x7", 1512, 7, 1, True, kernel=EXACT, px=8, aligned=1, col_blocks=3, block_cols=504),
    Row("fast_1512x9", 1512, 9, 3, False, kernel=FAST, px=8, aligned=1, col_blocks=3, block_cols=504),
    Row("exact_1008x7", 1008, 7, 4, True, kernel=EXACT, px=8, aligned=1, col_blocks=2, block_cols=504),
    Row("fast_1516x9", 1516, 9, 4, False, kernel=FAST, px=8, aligned=1, col_blocks=3, block_cols=504),
    # two bands of the exact kernel: 64 rows and one
    Row("exact_64x71", 64, 71, 3, True, kernel=EXACT, bands=2, aligned=1),
    Row("exact_509x71", 509, 71, 1, True, kernel=EXACT, bands=2, px=8, aligned=0),
    Row("exact_760x71", 760, 71, 1, True, kernel=EXACT, bands=2, px=4, aligned=1, col_blocks=4),
    Row("exact_1012x71", 1012, 71, 4, True, kernel=EXACT, bands=2, px=8, aligned=1, col_blocks=2),
    Row("exact_1010x71", 1010, 71, 3, True, kernel=EXACT, bands=2, px=8, aligned=0, col_blocks=2),
    # the fast kernel across a 14-row band seam: 23 rows = a band, a group of seven and two rows of the next
    Row("fast_1012x29", 1012, 29, 1, False, kernel=FAST, band_rows=14, bands=2, px=8, aligned=1, col_blocks=2),
    Row("fast_760x29", 760, 29, 3, False, kernel=FAST, band_rows=14, bands=2, px=4, aligned=1, col_blocks=4),
    Row("fast_1010x29", 1010, 29, 4, False, kernel=FAST, band_rows=14, bands=2, px=8, aligned=0, col_blocks=2),
    Row("fast_63x106", 63, 106, 1, False, kernel=FAST, band_rows=14, bands=8, px=4, aligned=0),
    # tall bands: by the pairs in the launch, which cycle through four image pairs
    Row("fast_64x132_p8192", 64, 132, 1, False, pairs=8192, distinct=4, kernel=FAST, band_rows=126, bands=1),
    Row("fast_64x132_p2048", 64, 132, 1, False, pairs=2048, distinct=4, kernel=FAST, band_rows=28, bands=5),
    Row("fast_64x132_p3200", 64, 132, 1, False, pairs=3200, distinct=4, kernel=FAST, band_rows=42, bands=3),   # G 7 equalised to 6
    Row("fast_64x134_p8192", 64, 134, 3, False, pairs=8192, distinct=4, kernel=FAST, band_rows=70, bands=2),   # G 18 equalised to 10
    # the lane seams inside a block, the right and the bottom edge
    Row("lanes_exact_64x7", 64, 7, 1, True, family="lanes", kernel=EXACT, px=4),
    Row("lanes_exact_509x8", 509, 8, 3, True, family="lanes", kernel=EXACT, px=8),
    Row("lanes_exact_1512x8", 1512, 8, 1, True, family="lanes", kernel=EXACT, px=8, aligned=1, col_blocks=3),
    Row("lanes_fast_64x90", 64, 90, 4, False, family="lanes", kernel=FAST, px=4),
    Row("lanes_fast_504x15", 504, 15, 1, False, family="lanes", kernel=FAST, px=4, col_blocks=2, why=BLOCKS),
    Row("lanes_fast_760x12", 760, 12, 3, False, family="lanes", kernel=FAST, px=4, aligned=1, col_blocks=4),
    Row("lanes_fast_512x17", 512, 17, 3, False, family="lanes", kernel=FAST, px=8),
    Row("lanes_fast_1010x12", 1010, 12, 1, False, family="lanes", kernel=FAST, px=8, col_blocks=2),
    Row("lanes_fast_1008x11", 1008, 11, 4, False, family="lanes", kernel=FAST, px=8, aligned=1, col_blocks=2),
    # five pairs of three waves each: the four waves of a workgroup belong to different pairs
    Row("shared_exact_756x7", 756, 7, 1, True, pairs=5, distinct=5, kernel=EXACT, items_per_pair=3),
    Row("shared_fast_756x12", 756, 12, 3, False, pairs=5, distinct=5, kernel=FAST, items_per_pair=3),
    # images in device memory at an address that is no multiple of 4
    Row("base1_64x90", 64, 90, 3, False, base=1, kernel=FAST, aligned=0, why=BASE),
    Row("base2_64x7", 64, 7, 1, True, base=2, kernel=EXACT, aligned=0, why=BASE),
    Row("base3_64x90", 64, 90, 4, False, base=3, kernel=FAST, aligned=0, why=BASE),
    Row("base1_512x7", 512, 7, 4, True, base=1, kernel=EXACT, px=8, aligned=0, why=BASE),
    Row("base2_512x15", 512, 15, 1, False, base=2, kernel=FAST, px=8, aligned=0, why=BASE),
    Row("base3_512x15", 512, 15, 3, False, base=3, kernel=FAST, px=8, aligned=0, why=BASE),
    Row("base1_63x78", 63, 78, 1, False, base=1, kernel=FAST, aligned=0, why=WIDTH),
    Row("base2_63x7", 63, 7, 3, True, base=2, kernel=EXACT, aligned=0, why=WIDTH),
    Row("base3_1011x11", 1011, 11, 1, False, base=3, kernel=FAST, px=8, aligned=0, col_blocks=2, why=WIDTH),
]
ROW = {r.name: r for r in ROWS}
assert len(ROW) == len(ROWS)
NAN_SHAPES = [(9, 6), (6, 9), (6, 6)]


def seams(row: Row) -> tuple:
    """(map columns, map rows) at which a block, or a band of either kernel, begins: the seam lies before each."""
    cols, rows = set(), set()
    for mode in (False, True):
        p = row.plan(mode)
        cols.update(k * p["block_cols"] for k in range(1, p["col_blocks"]))
        rows.update(k * p["band_rows"] for k in range(1, p["bands"]))
    return sorted(cols), sorted(rows)


def strength(row: Row) -> np.ndarray:
    """int[h, w]: 0, 1 or 2 -- how far b is from a at each pixel (the module's docstring)."""
    x, y = np.arange(row.w), np.arange(row.h)
    if row.family == "lanes":
        px = row.plan(row.exact)["px"]
        return (((x + 4) // px) % 2)[None, :] + (((y + 3) // 7) % 2)[:, None]
    cols, rows = seams(row)
    sx = sum((x >= c + 3).astype(np.int64) for c in cols) if cols else np.zeros(row.w, np.int64)
    sy = sum((y >= r + 3).astype(np.int64) for r in rows) if rows else np.zeros(row.h, np.int64)
    if not cols and not rows:                                # a single wave: the picture's own halves
        sx, sy = (x >= row.w // 2).astype(np.int64), (y >= row.h // 2).astype(np.int64)
    return (sx % 2)[None, :] + (sy % 2)[:, None]


def pixels(row: Row) -> np.ndarray:
    """uint8[2 * distinct, h, w(, channels)]: images 2k and 2k + 1 are pair k.  Seeded by the row's name."""
    rng = np.random.default_rng(zlib.crc32(row.name.encode()))
    shape = (row.distinct, row.h, row.w, row.channels)
    a = 128 + rng.choice([-1, 1], shape) * rng.integers(32, 49, shape)
    st = strength(row)
    g = np.array([1.0, 0.27, 0.0] if st.max() == 2 else [1.0, 0.0])[st]
    b = 128 + np.rint(g[None, :, :, None] * (a - 128)).astype(np.int64)
    px = np.stack([a, b], axis=1).reshape((2 * row.distinct,) + shape[1:]).astype(np.uint8)
    return px[..., 0].copy() if row.channels == 1 else px


def luma(px: np.ndarray) -> np.ndarray:
    """Pillow's convert("L") of RGB or RGBX pixels [..., 3 or 4] in integers; a luma plane passes through."""
    if px.ndim < 3 or px.shape[-1] not in (3, 4):
        return px
    c = px.astype(np.int64)
    return ((19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 0x8000) >> 16).astype(np.uint8)


def _box7(v: np.ndarray) -> np.ndarray:
    """Mean over every 7 x 7 window that lies inside v (float64)."""
    s = np.cumsum(np.pad(v, ((1, 0), (0, 0))), axis=0)
    s = s[7:] - s[:-7]
    s = np.cumsum(np.pad(s, ((0, 0), (1, 0))), axis=1)
    return (s[:, 7:] - s[:, :-7]) / 49.0


def ssim_map(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """skimage.metrics.structural_similarity's map of two luma planes (data_range 1, 7 x 7 uniform window, sample covariance),
    cropped to the windows that lie inside the image, in float64: the mean of it is the score."""
    x, y = a.astype(np.float64) / 255.0, b.astype(np.float64) / 255.0
    ux, uy = _box7(x), _box7(y)
    n = 49.0 / 48.0
    vx, vy, vxy = n * (_box7(x * x) - ux * ux), n * (_box7(y * y) - uy * uy), n * (_box7(x * y) - ux * uy)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
