"""Hand-written JPEG files for what lies BEHIND the entropy decoder (tests/_jpeg_write.py writes them, coefficient by
coefficient): the dequantisation and ke_idct_islow with its 16-bit bound, the upsampling of padded planes, the colour
conversion.  Files an encoder wrote from pictures stay far inside the bound, fill the padding of their planes by replication and
reach a small part of the (Y, Cb, Cr) cube; tests/_jpeg_stream_cases.py keeps its coefficients small on purpose.

  bound_cases()    blocks whose largest pass input lies just inside +-2^14 (taken, Pillow's pixels) or just outside (one such
                   block in an otherwise harmless file: handed back, status 1), in every component and at every block position
                   of an MCU, sequential and progressive; DC-only blocks of +-4095 / +-4096; three asymmetric quantisation
                   tables under ids 0, 1 and 3.
  padding_cases()  subsampled files of 1 x 1 .. 18 x 18 and around 256 / 512 columns whose padding (the columns and rows of the
                   planes beyond the component's real size, whole blocks of the MCU padding included) holds other values than
                   the last real column and row: a kernel that reads them instead of clamping shows.
  colour_cases()   4:4:4 files whose planes are ramps: every pair of two of Y, Cb, Cr.

  (name, file, facts) each; coverage() asserts from the coefficients and from Pillow alone that the families reach what they
  are for, and returns the figures.

extremes() restates what ke_idct_islow (csrc/ke_jpeg_core.h) tracks for its bound, in plain integers: it builds cases and
predicts statuses, it is never a pixel reference (that is Pillow).

Where the extreme can sit.  The column pass is 4 sqrt(8) times an orthonormal transform (a column that holds only i0 comes out
as 4 i0), so its largest result is at least four times its largest input, rounding aside: the largest value of a block is
always among the ROW pass's inputs, and a dequantised coefficient beyond 4 095 already puts the block outside (the lone AC of
16 383 and the DC of 4 096 below are handed back for what the row pass sees).  No block can have its extreme among the column
pass's inputs; what the cases do reach on that side is the ceiling of the column pass's inputs themselves, +-4 095
(coverage() asserts both facts)."""
from __future__ import annotations

import functools
import io
from types import SimpleNamespace

import numpy as np
from PIL import Image

import _jpeg_prog_encoder as E
import _jpeg_stream_cases as S
import _jpeg_write as W

# natural (row-major) index of zigzag position k: KE_ZZ
ZZ = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35,
      42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
BOUND = 1 << 14
TAKEN, BACK = (15000, BOUND - 1), (BOUND, 17500)
COUNTS, STEPS = (1, 2, 3, 6, 20), (1, 2, 4, 7, 255)


def _column(i0, i1, i2, i3, i4, i5, i6, i7):
    """ke_idct_islow's pass 1 on one column with AC: the eight results, descaled by 11."""
    z1 = (i2 + i6) * 4433
    tmp2, tmp3 = z1 - i6 * 15137, z1 + i2 * 6270
    tmp0, tmp1 = (i0 + i4) * 8192, (i0 - i4) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = i7, i5, i3, i1
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    sums = (tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3)
    return [(v + 1024) >> 11 for v in sums]


def extremes(block, steps):
    """block: 64 quantised coefficients, steps: 64 quantisation steps, both in zigzag order.  -> what ke_idct_islow's bound
    looks at: `column` / `row`, the largest |input| of either pass (the dequantised block; the column pass's results, with the
    shortcut for columns without AC), `largest` of the two, `value` (the signed value that reaches it), `dc_columns` /
    `dc_rows` (how many columns / rows take the passes' shortcuts).  The block is narrow iff largest < 2^14."""
    nat = [0] * 64
    for k in range(64):
        nat[ZZ[k]] = int(block[k]) * int(steps[k])
    assert max(map(abs, nat)) < 1 << 15, "outside the range this restatement (and 32-bit arithmetic) is meant for"
    ws, dc_columns = [0] * 64, 0
    for c in range(8):
        col = nat[c::8]
        if any(col[1:]):
            ws[c::8] = _column(*col)
        else:
            ws[c::8] = [col[0] * 4] * 8
            dc_columns += 1
    dc_rows = sum(1 for r in range(8) if not any(ws[8 * r + 1:8 * r + 8]))
    value = max(nat + ws, key=abs)
    return SimpleNamespace(column=max(map(abs, nat)), row=max(map(abs, ws)), largest=abs(value), value=value, dc_columns=dc_columns,
                           dc_rows=dc_rows)


def narrow(block, steps) -> bool:
    return extremes(block, steps).largest < BOUND


def _flat(step):
    return np.full(64, step, np.uint8)


def _search(rng, count, step, lo, hi, layout):
    """A random block of `count` non-zero coefficients at `step`, rescaled so that its extreme lies in lo..hi; None where the
    draw cannot get there (coefficients are kept within +-1023).  layout: "any", "column0" (natural positions 0, 8 .. 56: every
    row's AC part is zero, the row pass's shortcut) or "row0" (0 .. 7: every column's is, the column pass's)."""
    allowed = [k for k in range(64) if layout == "any" or (ZZ[k] % 8 == 0 if layout == "column0" else ZZ[k] < 8)]
    if count > len(allowed):
        return None
    q = _flat(step)
    b = np.zeros(64, np.int64)
    at = rng.choice(allowed, count, replace=False)
    b[at] = rng.integers(1, 101, count) * rng.choice([-1, 1], count)
    target = int((hi if lo < BOUND else lo) if rng.random() < 0.25 else rng.integers(lo, hi + 1))   # a quarter aim at the edge itself
    for _ in range(3):
        e = extremes(b, q).largest
        if lo <= e <= hi:
            break
        scaled = np.rint(b * (target / e)).astype(np.int64)
        if np.abs(scaled).max() > 1023 or np.count_nonzero(scaled) != count or np.abs(scaled * step).max() >= 1 << 15 or np.array_equal(scaled, b):
            return None
        b = scaled
    e = extremes(b, q)
    return (b.astype(np.int32), step, e) if lo <= e.largest <= hi else None


def _blocks(seed, lo, hi, per_cell):
    """per_cell blocks for every (count, step, layout) the search can serve."""
    rng = np.random.default_rng(seed)
    out = []
    for count in COUNTS:
        for step in STEPS:
            for layout, share in (("any", 1.0), ("column0", 0.25), ("row0", 0.25)):
                got = tries = 0
                want = max(1, int(per_cell * share))
                while got < want and tries < 6 * want:
                    tries += 1
                    found = _search(rng, count, step, lo, hi, layout)
                    if found:
                        out.append(found + (layout,))
                        got += 1
    return out


@functools.lru_cache(maxsize=None)
def taken_blocks():
    """(block, step, extremes, layout) of every block just inside the bound."""
    return tuple(_blocks(31, *TAKEN, 100))


@functools.lru_cache(maxsize=None)
def back_blocks():
    return tuple(_blocks(32, *BACK, 24))


def _benign(rng, shape, step):
    """Harmless blocks at `step`: far inside the bound (coverage() checks)."""
    a = np.zeros(shape + (64,), np.int32)
    a[..., 0] = rng.integers(-(400 // step), 400 // step + 1, shape)
    m = max(1, 30 // step)
    a[..., 1:] = rng.integers(-m, m + 1, shape + (63,)) * (rng.random(shape + (63,)) < 0.1)
    return a


def _tables(seed):
    return S.shaper("random2", "random3", seed)


def _facts(**kw):
    return SimpleNamespace(**kw)


def _write(name, w, h, sampling, coefs, q, seed, status, progressive=None, **more):
    comps = S.components(sampling)
    if progressive is None:
        data = W.write(w, h, comps, coefs, q, _tables(seed))[0]
    else:                                                           # the same coefficients through the same ke_jpeg_idct
        script = E.random_script(np.random.default_rng([33, seed]), len(comps))
        data = E.encode(w, h, [c[:3] for c in comps], coefs, script, [q[0], q[1]] if len(comps) > 1 else [q[0]])
    return name, data, _facts(status=status, sampling=sampling, size=(w, h), coefs=coefs, q=q, progressive=progressive is not None, **more)


def _dc_only():
    cases = []
    for value, step, status in ((819, 5, 0), (-819, 5, 0), (1024, 4, 1), (-1024, 4, 1)):
        a = np.zeros((2, 2, 64), np.int32)
        a[..., 0] = value
        cases.append(_write(f"bound_dc_only_{value * step}", 16, 16, "gray", [a], {0: _flat(step)}, 0, status))
    return cases


def _taken_files():
    """The taken blocks 16 to a 32 x 32 gray file (one quantisation step per file), and again in the Y, Cb and Cr components of
    4:4:4 (16 + 16 + 16 blocks) and 4:2:0 (16 + 4 + 4) files: every block of every MCU is one of them."""
    by_step = {s: [b for b in taken_blocks() if b[1] == s] for s in STEPS}
    gray, colour = [], []
    for step, blocks in by_step.items():
        for k in range(0, len(blocks) - 15, 16):
            a = np.stack([b[0] for b in blocks[k:k + 16]]).reshape(4, 4, 64)
            gray.append(_write(f"bound_taken_gray_step{step}_{k // 16}", 32, 32, "gray", [a], {0: _flat(step)}, len(gray), 0, blocks=blocks[k:k + 16]))
    rng = np.random.default_rng(34)
    for k in range(60):
        sampling = ("444", "420")[k % 2]
        sy, sc = STEPS[k // 2 % 5], STEPS[(k // 2 + 1 + k // 10) % 5]
        n = 16 if sampling == "444" else 4
        pick = lambda s, n: [by_step[s][int(j)] for j in rng.choice(len(by_step[s]), n, replace=False)]
        parts = [pick(sy, 16), pick(sc, n), pick(sc, n)]
        side = 4 if sampling == "444" else 2
        coefs = [np.stack([b[0] for b in parts[0]]).reshape(4, 4, 64)] + [np.stack([b[0] for b in p]).reshape(side, side, 64) for p in parts[1:]]
        colour.append(_write(f"bound_taken_{sampling}_steps{sy}_{sc}_{k}", 32, 32, sampling, coefs, {0: _flat(sy), 1: _flat(sc)}, 1000 + k, 0,
                             blocks=parts[0] + parts[1] + parts[2]))
    return gray, colour


PLACES = (("gray", 0), ("444", 0), ("444", 1), ("444", 2), ("420", 0), ("420", 1), ("420", 2))


def _back_files():
    """One block outside the bound per file -- in Y, Cb or Cr, as the first, a middle or the last block of its component --
    among harmless ones."""
    cases = []
    blocks = back_blocks()
    per = len(blocks) // (len(PLACES) * 3)
    assert per >= 15, len(blocks)
    order = np.random.default_rng(35).permutation(len(blocks))
    k = 0
    for sampling, c in PLACES:
        w, h = (48, 32) if sampling == "420" else (24, 16)
        comps = S.components(sampling)
        for where in ("first", "middle", "last"):
            for _ in range(per):
                block, step, e, layout = blocks[int(order[k])]
                rng = np.random.default_rng([36, k])
                q = {0: _flat(step if c == 0 else 1), 1: _flat(step if c else 1)}
                coefs = [_benign(rng, shape[:2], int(q[comps[j][3]][0])) for j, shape in enumerate(S.shapes_of(w, h, comps))]
                rows, cols = coefs[c].shape[:2]
                at = {"first": (0, 0), "middle": (rows // 2, cols // 2), "last": (rows - 1, cols - 1)}[where]
                coefs[c][at] = block
                cases.append(_write(f"bound_back_{sampling}_c{c}_{where}_{k}", w, h, sampling, coefs, q, 2000 + k, 1, blocks=[blocks[int(order[k])]],
                                    place=(c,) + at))
                k += 1
    return cases


def _transpose(q):
    """The table with its steps mirrored at the block's diagonal (zigzag order in and out)."""
    at = {ZZ[k]: k for k in range(64)}
    return np.array([q[at[(ZZ[k] % 8) * 8 + ZZ[k] // 8]] for k in range(64)], np.uint8)


def _table_files():
    """Three tables of 64 distinct steps each, none symmetric under transposition, under ids 0, 1 and 3: a decoder that reads a
    table in the wrong order, or another component's table, yields other pixels (coverage() asks Pillow)."""
    cases = []
    for k, (sampling, w, h) in enumerate((("444", 24, 16), ("420", 40, 24), ("422", 33, 17), ("440", 16, 35), ("444", 9, 9), ("420", 17, 17))):
        rng = np.random.default_rng([37, k])
        q = {t: (rng.permutation(64) + 1 + 30 * j).astype(np.uint8) for j, t in enumerate((0, 1, 3))}
        comps = S.components(sampling, tq=(0, 1, 3))
        coefs = []
        for c, shape in enumerate(S.shapes_of(w, h, comps)):
            a = (rng.integers(1, 3, shape) * rng.choice([-1, 1], shape) * (rng.random(shape) < 0.2)).astype(np.int32)
            a[..., 0] = rng.integers(-8, 9, shape[:2])
            coefs.append(a)
        data = W.write(w, h, comps, coefs, q, _tables(3000 + k))[0]
        cases.append((f"bound_tables_{sampling}_{w}x{h}", data, _facts(status=0, sampling=sampling, size=(w, h), coefs=coefs, q=q, comps=comps,
                                                                       progressive=False, tables=True)))
    return cases


@functools.lru_cache(maxsize=None)
def bound_cases():
    gray, colour = _taken_files()
    back = _back_files()
    prog = [_write(c[0] + "_progressive", *c[2].size, c[2].sampling, c[2].coefs, c[2].q, 4000 + k, c[2].status, progressive=True, blocks=c[2].blocks)
            for k, c in enumerate(gray[:100] + back[::len(back) // 50][:50])]
    return tuple(gray + colour + _dc_only() + back + prog + _table_files())


# ---- padding ---------------------------------------------------------------------------------------------------------------------------
SMALL = sorted({(w, h) for w in range(1, 19) for h in (1, 2, 3, 5, 8, 9, 15, 16, 17, 18)} | {(w, h) for h in range(1, 19) for w in (1, 2, 3, 4, 5, 7, 8, 9, 16, 17)})
WIDE = [(w, h) for w in (253, 255, 256, 257, 258, 259, 260, 261, 509, 513, 515) for h in (31, 33, 63, 65, 66)]


@functools.lru_cache(maxsize=None)
def padding_cases():
    """Every block of every plane, the blocks of the MCU padding included, drawn independently.  The wide sizes (the colour
    kernel's 256-column workgroups and 32-row groups) take the three samplings in turn, the control files (4:4:4, gray) every
    seventh size."""
    cases = []
    for k, (w, h) in enumerate(SMALL + WIDE):
        wide = w > 18
        samplings = [("422", "420", "440")[k % 3]] if wide else ["422", "420", "440"]
        if k % 7 == 0:
            samplings += ["444", "gray"]
        for sampling in samplings:
            rng = np.random.default_rng([41, k, list(S.FACTORS).index(sampling)])
            comps = S.components(sampling)
            coefs = S.coefficients(rng, w, h, comps, dc=900, ac=120, density=0.9)
            data = W.write(w, h, comps, coefs, S.steps(1, 1), _tables(5000 + k))[0]
            cases.append((f"padding_{sampling}_{w}x{h}", data, _facts(sampling=sampling, size=(w, h), coefs=coefs, comps=comps)))
    return tuple(cases)


# ---- colour --------------------------------------------------------------------------------------------------------------------------
PAIRS = ((1, 2), (0, 2), (0, 1))                                    # the two ramp planes: (Cb, Cr), (Y, Cr), (Y, Cb)


@functools.lru_cache(maxsize=None)
def colour_cases():
    """256 x 256 files at 4:4:4 that Pillow saves from a YCbCr array at quality 100: two planes are the x and the y ramp, the
    third is noise -- or all 0, all 255, all 128."""
    cases = []
    yy, xx = np.mgrid[0:256, 0:256]
    for k, (a, b) in enumerate(PAIRS):
        third = 3 - a - b
        for fill in ("noise", (128, 0, 255)[k]):                    # (Cb, Cr) under a Y of 128: G leaves 0..255 only at the far corners
            planes = [None] * 3
            planes[a], planes[b] = xx, yy
            planes[third] = np.random.default_rng([51, k]).integers(0, 256, (256, 256)) if fill == "noise" else np.full((256, 256), fill)
            buf = io.BytesIO()
            Image.fromarray(np.stack(planes, -1).astype(np.uint8), "YCbCr").save(buf, "JPEG", quality=100, subsampling=0)
            cases.append((f"colour_{'Y Cb Cr'.split()[a]}_{'Y Cb Cr'.split()[b]}_ramps_{fill}", buf.getvalue(), _facts(pair=(a, b), fill=fill)))
    return tuple(cases)


def ycc(data: bytes):
    """The samples in front of the colour conversion, upsampled, as Pillow (libjpeg) hands them out in draft mode."""
    with Image.open(io.BytesIO(data)) as im:
        if im.mode != "L":
            im.draft("YCbCr", im.size)
            assert im.mode == "YCbCr"
        return np.asarray(im)


@functools.lru_cache(maxsize=None)
def references():
    """{name: Pillow's pixels} of every case, computed once."""
    return {c[0]: S.pillow(c[1]) for c in bound_cases() + padding_cases() + colour_cases()}


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def _plane_edge_differs(facts):
    """From the coefficients: does a chroma plane hold, right beyond its real size, something else than its last real column
    or row?  None where no plane has anything beyond its component (8 x 15 at 4:4:0: chroma of 8 x 8, two rows of Y blocks).
    The chroma planes of these samplings are one block per MCU, so what lies beyond is the rest of the component's last block
    column / row: a float IDCT of the planes, and a difference of 8 levels, far beyond what its rounding could explain.  Whole
    blocks of padding only exist in the Y plane; they are drawn independently of their neighbours and compared as
    coefficients."""
    w, h = facts.size
    hs, vs = S.FACTORS[facts.sampling]
    k = np.arange(8)
    basis = np.cos((2 * k[:, None] + 1) * k[None, :] * np.pi / 16) * np.where(k == 0, np.sqrt(1 / 8), 0.5)[None, :]     # [sample][frequency]
    nat = np.argsort(np.array(ZZ))                                      # zigzag position of natural index
    cw, ch = -(-w // hs), -(-h // vs)
    rows, cols = -(-h // 8), -(-w // 8)
    y = facts.coefs[0]
    if cw == y.shape[1] * 8 // hs and ch == y.shape[0] * 8 // vs and cols == y.shape[1] and rows == y.shape[0]:
        return None
    for plane in facts.coefs[1:]:
        px = np.einsum("yv,rcvu,xu->rycx", basis, plane[:, :, nat].reshape(plane.shape[:2] + (8, 8)).astype(float), basis)
        px = np.clip(np.rint(px.reshape(plane.shape[0] * 8, plane.shape[1] * 8) + 128), 0, 255)
        if cw < px.shape[1] and np.abs(px[:ch, cw] - px[:ch, cw - 1]).max() >= 8:
            return True
        if ch < px.shape[0] and np.abs(px[ch, :cw] - px[ch - 1, :cw]).max() >= 8:
            return True
    return bool((cols < y.shape[1] and (y[:rows, cols] != y[:rows, cols - 1]).any()) or (rows < y.shape[0] and (y[rows, :cols] != y[rows - 1, :cols]).any()))


def coverage():
    """The families reach what they are for, judged from the coefficients and from Pillow alone.  -> the figures."""
    refs = references()
    fig = {}
    cases = bound_cases()
    used = {id(b[0]): b for c in cases if getattr(c[2], "blocks", None) for b in c[2].blocks}
    t = [b for b in used.values() if b[2].largest < BOUND]
    o = [b for b in used.values() if b[2].largest >= BOUND]
    assert len(t) >= 600 and all(TAKEN[0] <= b[2].largest <= TAKEN[1] for b in t), len(t)
    assert all(BACK[0] <= b[2].largest <= BACK[1] for b in o)
    for blocks in (t, o):
        assert {int(np.count_nonzero(b[0])) for b in blocks} == set(COUNTS) and {b[1] for b in blocks} == set(STEPS)
        assert {b[2].value > 0 for b in blocks} == {True, False}
        # both shortcuts, in all columns / rows of a block, in some columns, in none (a row loses its AC part only with all the others)
        assert any(b[2].dc_columns == 8 for b in blocks) and any(0 < b[2].dc_columns < 8 for b in blocks) and any(b[2].dc_columns == 0 for b in blocks)
        assert any(b[2].dc_rows == 8 for b in blocks) and any(b[2].dc_rows == 0 for b in blocks)
        # the extreme always sits among the row pass's inputs (see the module's docstring) ...
        assert all(b[2].largest == b[2].row and 4 * b[2].column <= b[2].row + 4 for b in blocks)
    # ... and the column pass's inputs reach their own ceiling, 4 095, on either sign
    assert max(b[2].column for b in t) >= 4090 and {int(c[2].coefs[0][0, 0, 0]) * int(c[2].q[0][0]) for c in cases if "dc_only" in c[0]} == {4095, -4095, 4096, -4096}
    assert any(b[1] == 255 and np.abs(b[0]).max() <= 16 for b in t)
    fig["taken_blocks"], fig["handed_back_blocks"] = len(t), len(o)
    fig["closest_inside"] = {"+": BOUND - max(b[2].value for b in t), "-": BOUND + min(b[2].value for b in t)}
    fig["closest_outside"] = {"+": max(0, min(b[2].value for b in o if b[2].value > 0) - BOUND), "-": max(0, -BOUND - max(b[2].value for b in o if b[2].value < 0))}
    # the pixels of the taken blocks are not merely saturated: a third of them show more than 8 values in Pillow's decode
    gray = [c for c in cases if c[0].startswith("bound_taken_gray") and not c[2].progressive]
    rich = sum(len(np.unique(refs[c[0]][8 * r:8 * r + 8, 8 * col:8 * col + 8])) > 8 for c in gray for r in range(4) for col in range(4))
    assert 3 * rich >= 16 * len(gray), (rich, len(gray))
    fig["taken_blocks_with_more_than_8_pixel_values"] = rich
    files = {key: [c for c in cases if c[0].startswith(key)] for key in ("bound_taken_gray", "bound_taken_444", "bound_taken_420", "bound_back", "bound_dc_only", "bound_tables")}
    sequential_back = [c for c in files["bound_back"] if not c[2].progressive]
    assert len(sequential_back) >= 300 and {c[2].place[0] for c in sequential_back} == {0, 1, 2}
    assert {(c[2].sampling, c[2].place[0], c[0].split("_")[4]) for c in sequential_back} == {(s, c, p) for s, c in PLACES for p in ("first", "middle", "last")}
    for c in sequential_back:                                       # exactly one block outside, the others far inside
        q = [c[2].q[0]] + [c[2].q[1]] * 2
        outside = [(j,) + at for j, plane in enumerate(c[2].coefs) for at in np.ndindex(plane.shape[:2]) if extremes(plane[at], q[j]).largest >= 8000]
        assert outside == [c[2].place], c[0]
    assert sum(c[2].progressive for c in files["bound_taken_gray"]) == 100 and sum(c[2].progressive for c in files["bound_back"]) == 50
    for c in files["bound_tables"]:
        f = c[2]
        assert all(len(set(q.tolist())) == 64 and not np.array_equal(_transpose(q), q) for q in f.q.values()) and set(f.q) == {0, 1, 3}
        assert all(narrow(plane[at], f.q[(0, 1, 3)[j]]) for j, plane in enumerate(f.coefs) for at in np.ndindex(plane.shape[:2]))
        for other in ({t: _transpose(q) for t, q in f.q.items()}, {0: f.q[1], 1: f.q[3], 3: f.q[0]}):
            wrong = S.pillow(W.write(*f.size, f.comps, f.coefs, other, _tables(0))[0])
            assert not np.array_equal(wrong, refs[c[0]]), c[0]
    fig["bound_files"] = {key: len(v) for key, v in files.items()}
    assert all(refs[c[0]] is not None for c in cases) and len({c[0] for c in cases}) == len(cases)

    pad = padding_cases()
    assert {c[2].size for c in pad if c[2].sampling in ("422", "420", "440")} == set(SMALL + WIDE)
    for s in ("422", "420", "440"):
        assert {c[2].size for c in pad if c[2].sampling == s} >= set(SMALL), s
    zero = full = step = padded = 0
    for name, data, facts in pad:
        if facts.sampling in ("gray", "444"):
            continue
        chroma = ycc(data)[:, :, 1:].astype(int)
        zero += bool((chroma == 0).any())
        full += bool((chroma == 255).any())
        step += bool(chroma.shape[1] > 1 and np.abs(np.diff(chroma, axis=1)).max() >= 100)
        hs, vs = S.FACTORS[facts.sampling]
        differs = _plane_edge_differs(facts)
        assert differs is not False, name
        padded += differs is True
    assert zero >= 100 and full >= 100 and step >= 100, (zero, full, step)
    fig["padding_files"] = len(pad)
    fig["padding"] = {"chroma_0": zero, "chroma_255": full, "chroma_step_100": step, "files_with_padding": padded}

    fig["colour_pairs"] = {}
    for name, data, facts in colour_cases():
        a, b = facts.pair
        s = ycc(data)
        pairs = np.unique(s[:, :, a].astype(np.int32) * 256 + s[:, :, b])
        if facts.fill == "noise":                                   # all 65 536 pairs; a Pillow that rounds otherwise: 99 % and the corners
            assert len(pairs) >= 0.99 * 65536 and {0, 255, 255 * 256, 255 * 256 + 255} <= set(pairs.tolist()), (name, len(pairs))
        fig["colour_pairs"][name] = len(pairs)
    return fig
