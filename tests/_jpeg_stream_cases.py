"""Hand-written JPEG entropy streams (tests/_jpeg_write.py): what other encoders and a hostile file can legally produce and
libjpeg-turbo's writer never does -- Huffman tables of chosen shapes, table and segment layouts, blocks written symbol by
symbol, stuffed FF 00 pairs / the end of the data / restart markers at chosen offsets, end-of-band runs of every size.

  valid()     (name, file, facts): the decoder must take every one of them, with Pillow's pixels.  The families are tables_,
              segments_, blocks_, stuffing_, ends_, restarts_, eobruns_ and prog_tables_; coverage() asserts from the writer's
              facts that each family reaches what it is for.
  tolerated() (name, file, status, why): streams libjpeg patches up without an error.  Pillow yields pixels, the decoder may
              refuse; `status` is what the host build gives, `why` names the line that causes it.  A taken file has Pillow's
              pixels.
  refused()   (name, file): unusable Huffman tables; status 2, and Pillow raises.  (A scan that names a table never defined is
              with the tolerated streams: libjpeg-turbo falls back to the standard tables for it.)

Coefficients stay inside ke_idct_islow's 16-bit bound (DC within +-900, AC within +-40 at a density of at most 0.3, steps of
at most 3, unless a case says otherwise and keeps the bound by other means) so that the decoder takes the file."""
from __future__ import annotations

import functools
import io
from collections import Counter

import numpy as np
from PIL import Image, ImageFile

import _jpeg_prog_encoder as E
import _jpeg_write as W

FACTORS = {"gray": None, "444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2)}
BIG = "eobruns_1456x1456_runs_of_16384_and_32767"


def pillow(data: bytes):
    """Pillow's pixels, or None where it raises (with LOAD_TRUNCATED_IMAGES off, whatever another test left it at)."""
    saved, ImageFile.LOAD_TRUNCATED_IMAGES = ImageFile.LOAD_TRUNCATED_IMAGES, False
    try:
        with Image.open(io.BytesIO(data)) as im:
            return np.asarray(im)
    except Exception:
        return None
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = saved


def components(sampling: str, ids=(1, 2, 3), tq=(0, 1, 1), td=(0, 1, 1), ta=(0, 1, 1)):
    if sampling == "gray":
        return [(ids[0], 1, 1, tq[0], td[0], ta[0])]
    hs, vs = FACTORS[sampling]
    return [(ids[0], hs, vs, tq[0], td[0], ta[0]), (ids[1], 1, 1, tq[1], td[1], ta[1]), (ids[2], 1, 1, tq[2], td[2], ta[2])]


def shapes_of(width, height, comps):
    hmax, vmax, mcus_x, mcus_y = W._geometry(width, height, comps)
    return [(mcus_y * (c[2] if len(comps) > 1 else 1), mcus_x * (c[1] if len(comps) > 1 else 1), 64) for c in comps]


def coefficients(rng, width, height, comps, mode="random", dc=900, ac=40, density=0.3):
    """mode: random / flat_dc (every DC 0: one DC symbol) / no_ac (one AC symbol) / few (coefficients 1..6 of every block set: no
    runs, a handful of AC symbols) / sparse (most blocks empty)."""
    out = []
    for shape in shapes_of(width, height, comps):
        a = np.zeros(shape, np.int32)
        if mode != "flat_dc":
            a[:, :, 0] = rng.integers(-dc, dc + 1, shape[:2])
        if mode == "few":
            a[:, :, 1:7] = rng.integers(1, ac + 1, shape[:2] + (6,)) * rng.choice([-1, 1], shape[:2] + (6,))
        elif mode == "sparse":
            a[:, :, 1:] = rng.integers(-3, 4, shape[:2] + (63,)) * (rng.random(shape[:2] + (63,)) < 0.04) * (rng.random(shape[:2] + (1,)) < 0.25)
        elif mode != "no_ac":
            a[:, :, 1:] = rng.integers(-ac, ac + 1, shape[:2] + (63,)) * (rng.random(shape[:2] + (63,)) < density * rng.random())
        out.append(a)
    return out


def steps(*values):
    return {k: np.full(64, v, np.uint8) for k, v in enumerate(values)}


def shaper(dc_shape: str, ac_shape: str, seed: int):
    """htables for W.write: the table of (scan, class, id) in the named shape, built on the symbols the scan draws from it."""
    def build(si, cls, tid, counter):
        name = ac_shape if cls else dc_shape
        dc = cls == 0
        syms = sorted(counter, key=lambda s: (-counter[s], s))
        syms = syms[tid % len(syms):] + syms[:tid % len(syms)] if name in ("all16", "full") else syms
        rng = np.random.default_rng([seed, si, cls, tid])
        if name == "ladder1":
            return W.ladder(syms, 1, dc)
        if name == "ladder5":
            return W.ladder(syms, 5, dc)
        if name == "ladder2":
            return W.ladder(syms, 2 + tid, dc)
        if name == "all16":
            return W.all_sixteen(syms, dc)
        if name == "edge":
            fill = [s for s in (range(12) if dc else range(0x11, 0x31)) if s not in counter]
            return W.edge_9_10(syms + fill[:max(0, 12 - len(syms))], dc)
        if name in ("single1", "single16"):
            assert len(syms) == 1
            return W.single(syms[0], 1 if name == "single1" else 16)
        if name == "full":
            return W.dc_full(syms, 16 if tid % 2 else 12) if dc else W.full_256(syms)
        if name == "inverted":
            return W.inverted(counter, dc)
        if name.startswith("random"):
            return W.random(rng, syms, int(name[6:]), dc)
        raise ValueError(name)
    return build


def _name(*parts):
    return "_".join(str(p) for p in parts)


# ---- V: valid files ----------------------------------------------------------------------------------------------------------------
SHAPES = (("ladder1", "ladder1", "few"), ("ladder5", "ladder5", "random"), ("all16", "all16", "random"), ("edge", "edge", "random"),
          ("single1", "random2", "flat_dc"), ("single16", "ladder2", "flat_dc"), ("random3", "single1", "no_ac"), ("ladder2", "single16", "no_ac"),
          ("full", "full", "random"), ("inverted", "inverted", "random"), ("random1", "random1", "random"), ("random5", "random9", "random"))
LAYOUTS = (("shared", (0, 0, 0), (0, 0, 0)), ("ids012", (0, 1, 2), (0, 1, 2)), ("ids123", (1, 2, 3), (1, 2, 3)), ("pair", (0, 1, 1), (0, 1, 1)))


def _tables():
    cases = []
    samplings = ("gray", "444", "422", "420", "440")
    k = 0
    for si, (dcs, acs, mode) in enumerate(SHAPES):
        for rep in range(3):
            sampling = samplings[k % 5]
            layout, td, ta = LAYOUTS[(k // 2) % 4]
            rng = np.random.default_rng([11, k])
            w, h = int(rng.integers(9, 97)), int(rng.integers(9, 81))
            comps = components(sampling, td=td, ta=ta)
            coefs = coefficients(rng, w, h, comps, mode)
            data, facts = W.write(w, h, comps, coefs, steps(1, 2), shaper(dcs, acs, k))
            facts.census = Counter({"sampling_" + sampling: 1, "layout_" + layout: sampling != "gray", "dc_" + dcs: 1, "ac_" + acs: 1})
            cases.append((_name("tables", dcs, acs, sampling, layout, f"{w}x{h}"), data, facts))
            k += 1
    return cases


def _segments():
    cases = []
    ids = ((0, 1, 2), (10, 200, 33), (82, 71, 65))
    for k in range(24):
        rng = np.random.default_rng([12, k])
        gray = k % 4 == 3
        sampling = "gray" if gray else ("444", "422", "420", "440")[k % 3 + (k % 5 == 0)]
        tq = ((0, 1, 1), (1, 2, 3), (3, 0, 2), (2, 2, 2))[k % 4]
        comps = components(sampling, ids=ids[k % 3], tq=tq, td=(0, 1, 1) if k % 2 else (1, 2, 3), ta=(0, 1, 1) if k % 2 else (1, 0, 3))
        w, h = int(rng.integers(9, 97)), int(rng.integers(9, 81))
        opts = dict(dht_layout=("each", "one")[k % 2], dht_behind_sof=bool(k // 2 % 2), dht_twice=k % 3 == 0, extra_tables=k % 4 == 1,
                    dqt_behind_sof=bool(k // 4 % 2), sof=0xC1 if k % 3 == 1 else 0xC0, jfif=k % 5 != 2,
                    adobe_transform=1 if (k % 5 in (2, 3) and not gray) else None,
                    frame_factors=[0x22] if gray and k % 8 == 3 else None, leading=W.com(int(rng.integers(4, 40))) if k % 2 else W.segment(0xE5, b"x" * (k + 1)))
        q = {t: np.full(64, 1 + (t + k) % 3, np.uint8) for t in set(tq[:len(comps)])}
        data, facts = W.write(w, h, comps, coefficients(rng, w, h, comps), q, shaper("random2", "random3", 100 + k), **opts)
        facts.census = Counter({f"dht_{opts['dht_layout']}": 1, f"dht_behind_sof_{opts['dht_behind_sof']}": 1, "dht_twice": opts["dht_twice"],
                                "extra_tables": opts["extra_tables"], f"dqt_behind_sof_{opts['dqt_behind_sof']}": 1, "sof1": opts["sof"] == 0xC1,
                                f"ids_{ids[k % 3][0]}": not gray, "tq_3": 3 in tq[:len(comps)], "adobe_without_jfif": opts["adobe_transform"] == 1 and not opts["jfif"],
                                "adobe_with_jfif": opts["adobe_transform"] == 1 and opts["jfif"], "gray_2x2": opts["frame_factors"] is not None})
        cases.append((_name("segments", k, sampling, f"{w}x{h}"), data, facts))
    return cases


def _dc_walk():
    """DC values whose differences are of every category 0..11 at both ends of the category, either sign, inside -1024..1023."""
    values, cur = [], 0
    for s in range(12):
        for d in sorted({0} if s == 0 else {1 << (s - 1), (1 << s) - 1, -(1 << (s - 1)), -((1 << s) - 1)}):
            if not -1024 <= cur + d <= 1023:
                cur = -1024 if d > 0 else 1023                 # a block in between that makes room
                values.append(cur)
            cur += d
            values.append(cur)
    return values


def _blocks():
    cases = []

    def gray(name, blocks, zrl_tail=0, dc="ladder2", ac="random2", seed=0, step=1):
        n = len(blocks)
        cols = min(n, 12)
        rows = -(-n // cols)
        a = np.zeros((rows, cols, 64), np.int32)
        a.reshape(-1, 64)[:n] = blocks
        data, facts = W.write(cols * 8 - 3, rows * 8 - 2, components("gray"), [a], steps(step), shaper(dc, ac, 200 + seed), zrl_tail=zrl_tail)
        facts.census = Counter({name: 1})
        cases.append(("blocks_" + name, data, facts))

    def blk(**at):
        b = np.zeros(64, np.int32)
        for k, v in at.items():
            b[int(k[1:])] = v
        return b

    rng = np.random.default_rng(13)
    gray("coefficient_63_set_no_eob", [blk(k0=50, k63=3), blk(k0=40, k1=-2, k63=-1), blk(k0=30, k62=1, k63=1), blk(k0=10)])
    gray("run_of_15_ends_on_63", [blk(k0=5, k47=2, k63=-3), blk(k0=-7, k47=-1, k63=1)])
    gray("two_and_three_zrls", [blk(k0=1, k33=4), blk(k0=2, k40=-4, k63=1), blk(k0=3, k49=7), blk(k0=4, k60=-9), blk(k0=5, k1=1, k50=2)])
    for tail in (1, 2, 3):
        gray(f"zrl_chain_{tail}_in_front_of_eob", [blk(k0=9), blk(k0=8, k1=3), blk(k0=7, k14=-2), blk(k0=6, k15=2), blk(k0=5, k30=1), blk(k0=4, k31=1),
                                                    blk(k0=3, k46=-1), blk(k0=2, k47=5), blk(k0=1, k62=1)], zrl_tail=tail, seed=tail)
    gray("all_zero_blocks", [np.zeros(64, np.int32)] * 30, dc="single1", ac="single1")
    gray("all_zero_blocks_16_bit_codes", [np.zeros(64, np.int32)] * 30, dc="single16", ac="single16")
    full = rng.integers(1, 4, (6, 64)) * rng.choice([-1, 1], (6, 64))
    full[:, 0] = (100, -100, 0, 50, 51, 49)
    gray("every_position_set", list(full), ac="ladder1")
    sizes = []
    for s in range(1, 11):                                         # both ends of every AC size, either sign, one per block (the bound holds)
        for v in (1 << (s - 1), (1 << s) - 1):
            sizes += [blk(k0=0, **{f"k{1 + (s * 5) % 62}": v}), blk(k0=0, **{f"k{2 + (s * 7) % 61}": -v})]
    gray("ac_sizes_1_to_10", sizes, ac="random4")
    walk = _dc_walk()
    gray("dc_categories_0_to_11", [blk(k0=v) for v in walk], dc="ladder5")
    gray("dc_categories_0_to_11_inverted", [blk(k0=v) for v in walk], dc="inverted", ac="single16")
    return cases


def _stuffing():
    """Magnitude bits of all ones (coefficients 2^s - 1) behind codes that begin with ones (the long codes of a ladder)."""
    cases = []
    for k, n in enumerate(list(range(0, 68)) + [0, 5, 6, 7]):
        n = n if n == 0 or n >= 4 else n + 64                       # a COM segment is 4 bytes at least: 1..3 -> 65..67
        rng = np.random.default_rng([14, k])
        w, h = int(rng.integers(17, 57)), int(rng.integers(17, 41))
        comps = components("gray")
        a = np.zeros(shapes_of(w, h, comps)[0], np.int32)
        a[:, :, 0] = np.cumsum(rng.choice([127, 255, -127, 63, 0], a.shape[:2]).ravel()).reshape(a.shape[:2]) % 1800 - 900
        a[:, :, 1:] = rng.choice([0, 1, 3, 7, 15, 31, 63], a.shape[:2] + (63,), p=[.8, .02, .03, .03, .04, .04, .04])
        if k >= 68:
            a[-1, -1, 40:] = 0
            a[-1, -1, 63] = (1023, 511, 255, 127)[k - 68]           # the last bits of the stream: ones, a stuffed pair ends the data
            a[-1, -1, 0] = 0
        # the symbols used most get the LONGEST codes of a ladder from 1: 1...10 prefixes in front of all-ones magnitudes
        def tabs(si, cls, tid, counter):
            syms = sorted(counter, key=lambda s: (counter[s], s))
            return W.ladder(syms, max(1, 17 - len(syms)) if len(syms) <= 16 else 6, cls == 0)
        data, facts = W.write(w, h, comps, [a], steps(1), tabs, leading=W.com(n))
        facts.census = Counter({f"com_{n}": 1})
        cases.append((_name("stuffing", k, f"com{n}", f"{w}x{h}"), data, facts))
    return cases


def _fixed(dc_len, ac_len):
    return lambda si, cls, tid, counter: W.table(sorted(counter), [ac_len if cls else dc_len] * len(counter))


def _ends():
    cases = []

    def flat(name, blocks, dc_len, ac_len, com=0, pad_ones=True, **kw):
        cols = blocks if blocks <= 16 else 15 if blocks % 15 == 0 else 16
        a = [np.zeros((blocks // cols, cols, 64), np.int32)]
        data, facts = W.write(cols * 8, blocks // cols * 8, components("gray"), a, steps(1), _fixed(dc_len, ac_len), leading=W.com(com), pad_ones=pad_ones, **kw)
        facts.census = Counter({name: 1})
        cases.append((_name("ends", name, f"com{com}"), data, facts))

    for blocks in range(1, 17):                                     # a byte a block: the EOI at every one of a lane's 16 positions in
        for com in (0, 5):                                          # ke_jpeg_find_end, counted from the scan's first aligned dword
            flat(f"eoi_mod_16_{blocks}_bytes", blocks, 3, 5, com)
    for blocks in (255, 256):                                       # 4 bytes a block: the EOI on either side of 1 024 bytes from the
        for com in (0, 4, 5, 6, 7):                                 # first aligned dword, in steps of one byte
            flat(f"eoi_at_step_edge_{blocks}", blocks, 16, 16, com)
    for total, (blocks, dc_len, ac_len) in {1: (1, 1, 1), 2: (1, 7, 5), 3: (1, 1, 16), 4: (1, 16, 16), 5: (2, 16, 4), 8: (2, 16, 16)}.items():
        for com in (0, 5, 6, 7):
            flat(f"data_of_{total}_bytes", blocks, dc_len, ac_len, com)
    for pad in range(8):
        for ones in (True, False):
            flat(f"pad_{pad}_bits_of_{'ones' if ones else 'zeros'}", 1, 8, 8 - pad, pad_ones=ones)
    flat("bytes_between_data_and_eoi", 5, 3, 4, before_marker={"eoi": b"\x12\x00\x34"})
    flat("one_byte_between_data_and_eoi", 2, 16, 16, before_marker={"eoi": b"\x7f"})
    rng = np.random.default_rng(15)
    for k in range(6):                                              # ... and the same edges on real data
        w, h = int(rng.integers(30, 97)), int(rng.integers(30, 81))
        comps = components(("gray", "420", "444")[k % 3])
        data, facts = W.write(w, h, comps, coefficients(rng, w, h, comps), steps(2, 3), shaper("random2", "random2", 300 + k), leading=W.com(4 + k),
                              pad_ones=bool(k % 2))
        facts.census = Counter({"random_data": 1})
        cases.append((_name("ends_random", k, f"{w}x{h}"), data, facts))
    return cases


PROG_RESTART_SCRIPT = {1: [([0], 0, 0, 0, 1), ([0], 1, 5, 0, 1), ([0], 6, 63, 0, 1), ([0], 0, 0, 1, 0), ([0], 1, 5, 1, 0), ([0], 6, 63, 1, 0)],
                       3: [([0, 1, 2], 0, 0, 0, 1), ([0], 1, 63, 0, 1), ([2], 1, 63, 0, 0), ([1], 1, 9, 0, 2), ([1], 10, 63, 0, 0), ([1, 2], 0, 0, 1, 0),
                           ([0], 0, 0, 1, 0), ([1], 1, 9, 2, 1), ([0], 1, 63, 1, 0), ([1], 1, 9, 1, 0)]}


def _restarts():
    cases = []
    one_bit = lambda si, cls, tid, counter: W.single(next(iter(counter)), 1)
    for w, h, ones in ((48, 40, True), (48, 40, False), (200, 8, True)):      # MCUs of two bits: a marker every third byte
        a = [np.zeros((h // 8, w // 8, 64), np.int32)]
        data, facts = W.write(w, h, components("gray"), a, steps(1), one_bit, restart=1, pad_ones=ones)
        facts.census = Counter({"interval_1_flat": 1, "pad_zeros": not ones})
        cases.append((_name("restarts_flat_interval_1", f"{w}x{h}", "ones" if ones else "zeros"), data, facts))
    k = 0
    for sampling in ("gray", "420", "422", "444"):
        for what in ("1", "2", "row", "count", "beyond", "zero_behind", "random"):
            for prog in (False, True):
                rng = np.random.default_rng([16, k])
                k += 1
                w, h = int(rng.integers(33, 97)), int(rng.integers(25, 81))
                comps = components(sampling, td=(0, 1, 2), ta=(0, 1, 1))
                hmax, vmax, mx, my = W._geometry(w, h, comps)
                # (progressive: every scan counts its own MCUs -- single blocks in an AC scan; the interval is the frame's)
                ri = {"1": 1, "2": 2, "row": mx, "count": mx * my, "beyond": mx * my + 3, "zero_behind": 0, "random": int(rng.integers(1, 12))}[what]
                kw = dict(restart=ri, pad_ones=bool(k % 3), leading=W.com(4 + k % 9))
                if what == "zero_behind":
                    kw["dri"] = [7, 0]
                coefs = coefficients(rng, w, h, comps)
                if prog:
                    script = PROG_RESTART_SCRIPT[len(comps)]
                    data, facts = W.write(w, h, comps, coefs, steps(2, 1), shaper("random2", "random2", 400 + k), sof=0xC2, script=script,
                                          max_eobrun=(1, 5, 32767)[k % 3], **kw)
                    kinds = Counter()
                    for si, s in enumerate(script):                   # which kinds of scan hold a restart marker
                        lo, hi = facts.scan_offsets[si], facts.scan_ends[si]
                        kinds[("dc" if s[1] == 0 else "ac") + ("_refine" if s[3] else "_first") + "_crosses_restart"] += any(lo <= p < hi for p in facts.restarts)
                else:
                    data, facts = W.write(w, h, comps, coefs, steps(2, 1), shaper("random2", "random2", 400 + k), **kw)
                    kinds = Counter()
                facts.census = kinds + Counter({"interval_" + what: 1, "pad_zeros": not kw["pad_ones"], "progressive": prog})
                cases.append((_name("restarts", sampling, what, "prog" if prog else "seq", f"{w}x{h}"), data, facts))
    return cases


def _scan_tables(kind):
    """Tables that hold only the symbols a scan uses: single / ladder shapes, or everything at 16 bits."""
    def build(si, cls, tid, counter):
        syms = sorted(counter, key=lambda s: (-counter[s], s))
        if kind == "all16":
            return W.all_sixteen(syms, cls == 0)
        return W.single(syms[0], 1) if len(syms) == 1 else W.ladder(syms, 1 if len(syms) <= 16 else 3, cls == 0)
    return build


def _eobruns():
    cases = []
    script = [([0], 0, 0, 0, 0), ([0], 1, 5, 0, 2), ([0], 6, 63, 0, 1), ([0], 1, 5, 2, 1), ([0], 6, 63, 1, 0), ([0], 1, 5, 1, 0)]
    for limit in (1, 2, 3, 4, 7, 8, 255, 256, 32767):
        for kind in ("ladder", "all16"):
            for ri in (0, 23):
                rng = np.random.default_rng([17, limit])
                w, h = (136, 128) if limit >= 255 else (int(rng.integers(60, 97)), int(rng.integers(50, 81)))
                comps = components("gray")
                coefs = coefficients(rng, w, h, comps, "sparse")
                coefs[0][:, :, 1:4] += (rng.random(coefs[0].shape[:2] + (3,)) < 0.08) * 6     # coefficients the refinement scans correct inside a run
                coefs[0][-3:, :, 1:] = 0                              # the last blocks are empty: a run ends on the last block
                if limit >= 255:                                      # 257 empty blocks behind the first 15
                    coefs[0].reshape(-1, 64)[15:, 1:] = 0
                data, facts = W.write(w, h, comps, coefs, steps(2), _scan_tables(kind), sof=0xC2, script=script, max_eobrun=limit, restart=ri)
                facts.census = Counter({f"limit_{limit}": 1, "tables_" + kind: 1, "restarts": bool(ri)})
                cases.append((_name("eobruns", f"limit{limit}", kind, f"ri{ri}", f"{w}x{h}"), data, facts))
    # one flat gray file of 182 x 182 = 33 124 blocks: gaps of 1, 2, 4 ... 16 384 empty blocks between the few that hold a coefficient
    # of the first band (EOB0 .. EOB14 in one scan), a second band that is empty throughout (a run of 32 767, then the rest)
    a = np.zeros((182, 182, 64), np.int32)
    flatv = a.reshape(-1, 64)
    at = 0
    for n in range(15):
        flatv[at, 1] = 1 + n % 3
        flatv[at, 2] = -2
        at += 1 + (1 << n)                                          # a run of 2^n empty blocks: EOBn with extra bits of zeros
    assert at < 33124 - 300, at
    flatv[at, 1] = 5
    flatv[:, 0] = 40
    big = [([0], 0, 0, 0, 0), ([0], 1, 2, 0, 1), ([0], 3, 63, 0, 0), ([0], 1, 2, 1, 0)]
    data, facts = W.write(1456, 1456, components("gray"), [a], steps(1), _scan_tables("ladder"), sof=0xC2, script=big, max_eobrun=32767)
    facts.census = Counter({"big": 1})
    cases.append((BIG, data, facts))
    return cases


def _prog_tables():
    cases = []
    for k, (dcs, acs, mode) in enumerate(SHAPES):
        if "single" in dcs + acs or "ladder1" in dcs + acs:           # a scan's band decides its symbols: no one-symbol tables and no
                                                                      # ladder from 1 bit here; other shapes take their turn
            dcs, acs = ("random1", "ladder2") if k % 2 else ("ladder2", "random4")
        for rep in range(2):
            rng = np.random.default_rng([18, k, rep])
            sampling = ("gray", "444", "422", "420", "440")[(2 * k + rep) % 5]
            w, h = int(rng.integers(9, 90)), int(rng.integers(9, 70))
            comps = components(sampling, td=(0, 1, 2), ta=(0, 1, 2) if rep else (3, 3, 3))   # DC scans: one table per component
            script = E.random_script(rng, len(comps))
            coefs = coefficients(rng, w, h, comps)
            data, facts = W.write(w, h, comps, coefs, steps(2, 3), shaper(dcs, acs, 500 + k), sof=0xC2, script=script, max_eobrun=(32767, 1, 6)[k % 3],
                                  restart=(0, 0, 9)[(k + rep) % 3])
            facts.census = Counter({"dc_" + dcs: 1, "ac_" + acs: 1, "sampling_" + sampling: 1})
            cases.append((_name("prog_tables", dcs, acs, sampling, f"{len(script)}scans", f"{w}x{h}"), data, facts))
    return cases


FAMILIES = {"tables": _tables, "segments": _segments, "blocks": _blocks, "stuffing": _stuffing, "ends": _ends, "restarts": _restarts,
            "eobruns": _eobruns, "prog_tables": _prog_tables}


@functools.lru_cache(maxsize=None)
def family(name: str):
    return tuple(FAMILIES[name]())


@functools.lru_cache(maxsize=None)
def valid():
    return tuple(c for name in FAMILIES for c in family(name))


@functools.lru_cache(maxsize=None)
def references():
    """{name: Pillow's pixels} of every valid and tolerated case, computed once."""
    return {c[0]: pillow(c[1]) for c in valid() + tolerated()}


def _lengths(cases, cls):
    total = Counter()
    for _, _, facts in cases:
        for (si, c, tid), cnt in facts.lengths.items():
            if c == cls:
                total += cnt
    return total


def window_offsets(facts):
    """Where the stuffed pairs of the first scan lie relative to its first aligned dword (the origin of the reader's window)."""
    origin = facts.scan_offsets[0] & ~3
    return [p - origin for p in facts.stuffed if p < facts.scan_ends[0]]


def device_reader(data: bytes, facts):
    """A model of how ke_jpeg.hip's sequential kernel pulls the first scan through its lane's window (bits_fill, stream_dword,
    stream_byte; no restarts): the reader refills before every Huffman symbol while it holds 32 bits or fewer -- four bytes at
    once where the dword at its position holds no 0xFF, one byte the careful way otherwise -- and the 64-byte window is loaded
    anew, at the position's dword, when a dword is wanted beyond offset 56 or a byte beyond 63.
    -> (window offsets at which the 0xFF of a stuffed pair was read, byte lanes of the tested dwords that held a 0xFF,
    stuffed pairs whose 0x00 was read from a window loaded after the 0xFF)."""
    pos, end = facts.scan_offsets[0], facts.scan_ends[0]
    win, n, offsets, lanes, split = pos & ~3, 0, [], set(), 0
    for bits in facts.reads[0]:
        while n <= 32:
            if pos + 4 <= end:
                if pos - win > 56:
                    win = pos & ~3
                w = data[pos:pos + 4]
                if 0xFF not in w:
                    n, pos = n + 32, pos + 4
                    continue
                lanes |= {k for k in range(4) if w[k] == 0xFF}
            if pos < end:
                if pos - win >= 64:
                    win = pos & ~3
                if data[pos] == 0xFF:                        # (inside the data every 0xFF is a stuffed pair's)
                    assert data[pos + 1] == 0 and pos + 1 < end
                    offsets.append(pos - win)
                    if pos + 1 - win >= 64:
                        win, split = (pos + 1) & ~3, split + 1
                    pos += 2
                else:
                    pos += 1
            n += 8
        n -= bits
        assert n >= 0
    return offsets, lanes, split


def coverage():
    """Every family reaches what it is for; -> {family: number of cases}."""
    t = family("tables")
    census = sum((c[2].census for c in t), Counter())
    for dcs, acs, _ in SHAPES:
        assert census["dc_" + dcs] and census["ac_" + acs], (dcs, acs)
    for key in ("sampling_gray", "sampling_444", "sampling_422", "sampling_420", "sampling_440", "layout_shared", "layout_ids012", "layout_ids123"):
        assert census[key], key
    assert set(_lengths(t, 0)) == set(range(1, 17)) and set(_lengths(t, 1)) == set(range(1, 17))
    assert any(sum(n for l, n in _lengths([c], 1).items() if l >= 10) * 2 > sum(_lengths([c], 1).values()) for c in t)
    edge = [c[2] for c in t if "_edge_" in c[0]]
    for facts in edge:                                              # the largest 9-bit code and the 10-bit one right behind it are decoded
        for key, tab in facts.tables.items():
            assert facts.symbols[key][tab.marks["last9"]] and facts.symbols[key][tab.marks["first10"]], key
            (c9, l9), (c10, l10) = tab.codes[tab.marks["last9"]], tab.codes[tab.marks["first10"]]
            assert (l9, l10) == (9, 10) and c10 == (c9 + 1) << 1
    assert any(len(c[2].tables[key].syms) == 256 for c in t for key in c[2].tables) and {12, 16} <= {len(c[2].tables[key].syms) for c in t for key in c[2].tables if key[1] == 0}
    assert any(len({id(v) for v in c[2].tables.values()}) == 6 for c in t)
    census = sum((c[2].census for c in family("segments")), Counter())
    for key in ("dht_each", "dht_one", "dht_behind_sof_True", "dht_behind_sof_False", "dht_twice", "extra_tables", "dqt_behind_sof_True", "dqt_behind_sof_False",
                "sof1", "ids_0", "ids_10", "ids_82", "tq_3", "adobe_without_jfif", "adobe_with_jfif", "gray_2x2"):
        assert census[key], key
    b = {c[0]: c[2] for c in family("blocks")}
    assert set(range(12)) <= set(b["blocks_dc_categories_0_to_11"].symbols[(0, 0, 0)])
    assert {(r << 4) | s for r in (0,) for s in range(1, 11)} <= {s & 0x0F for s in b["blocks_ac_sizes_1_to_10"].symbols[(0, 1, 0)]} | {0}
    assert b["blocks_two_and_three_zrls"].symbols[(0, 1, 0)][0xF0] >= 2 + 2 + 3 + 3 + 3
    assert b["blocks_run_of_15_ends_on_63"].symbols[(0, 1, 0)][0x00] == 0 and b["blocks_coefficient_63_set_no_eob"].symbols[(0, 1, 0)][0x00] == 1
    assert b["blocks_zrl_chain_3_in_front_of_eob"].symbols[(0, 1, 0)][0xF0] == (3 + 3 + 3 + 2 + 2 + 1 + 1) + (1 + 1 + 2 + 2 + 3)   # in front of the EOB as many as stay below 64; inside the runs
    assert b["blocks_every_position_set"].symbols[(0, 1, 0)][0x00] == 0
    s = [c[2] for c in family("stuffing")]
    offsets = [o for f in s for o in window_offsets(f)]
    assert {o % 56 for o in offsets} == set(range(56)) and {o % 64 for o in offsets} == set(range(64))
    # ... and where the reader really stands (device_reader): the window is loaded anew wherever a dword is wanted beyond offset 56,
    # so the 0xFF of a pair is met at offsets 0..56 -- all of them here -- and beyond only in the last three bytes of the data,
    # where no dword is read any more (at 62 at the most: its 0x00 is never in another window, a pair is never split across a
    # refill, and the model counts none); the dword that sends the reader down the byte path holds a 0xFF in each of its four lanes
    met, lanes, split = Counter(), set(), 0
    for c in family("stuffing"):
        o, l, n = device_reader(c[1], c[2])
        met.update(o)
        lanes |= l
        split += n
        assert len(o) == len(c[2].stuffed)
    assert set(range(57)) <= set(met) and max(met) <= 62 and lanes == {0, 1, 2, 3} and split == 0
    assert {f.scan_offsets[0] % 4 for f in s} == {0, 1, 2, 3}
    assert any(q - p == 2 for f in s for p, q in zip(f.stuffed, f.stuffed[1:]))
    assert sum(1 for f in s if f.stuffed and f.stuffed[-1] + 2 == f.scan_ends[0]) >= 2
    e = family("ends")
    assert {(c[2].eoi - (c[2].scan_offsets[0] & ~3)) % 16 for c in e if "eoi_mod_16" in c[0]} == set(range(16))
    assert {(c[2].eoi - (c[2].scan_offsets[0] & ~3)) % 1024 for c in e if "step_edge" in c[0]} >= {1020, 1021, 1022, 1023, 0, 1, 2, 3}
    assert {c[2].scan_ends[0] - c[2].scan_offsets[0] for c in e if "data_of" in c[0]} == {1, 2, 3, 4, 5, 8}
    for c in e:
        if "data_of" in c[0]:
            assert f"data_of_{c[2].scan_ends[0] - c[2].scan_offsets[0]}_bytes" in c[0]
    assert {(c[2].pad_bits[-1], "ones" in c[0]) for c in e if "_pad_" in c[0]} == {(p, o) for p in range(8) for o in (True, False)}
    r = family("restarts")
    census = sum((c[2].census for c in r), Counter())
    for key in ("interval_1_flat", "pad_zeros", "interval_1", "interval_2", "interval_row", "interval_count", "interval_beyond", "interval_zero_behind", "progressive",
                "dc_first_crosses_restart", "dc_refine_crosses_restart", "ac_first_crosses_restart", "ac_refine_crosses_restart"):
        assert census[key], key
    for c in r:
        if "flat_interval_1" in c[0]:                              # RST7 is followed by RST0 twice; a marker every third byte
            assert len(c[2].restarts) >= 20 and all(q - p == 3 for p, q in zip(c[2].restarts, c[2].restarts[1:]))
    eo = family("eobruns")
    runs = Counter(n.bit_length() - 1 for c in eo for n in c[2].eobruns)
    assert set(runs) == set(range(15)), runs
    big = [c for c in eo if c[0] == BIG][0][2]
    assert 16384 in big.eobruns and 32767 in big.eobruns
    for limit in (1, 2, 3, 4, 7, 8, 255, 256):
        assert any(max(c[2].eobruns) == limit for c in eo if f"limit{limit}_" in c[0]), limit
    assert any(p > 0 and n > 1 for c in eo for n, p in zip(c[2].eobruns, c[2].eobrun_pending))       # correction bits wait behind a run
    for limit in (2, 3, 4, 7, 8, 255, 256, 32767):                  # a run ends on the last block of a scan (one of 1 is never left over)
        assert any(c[2].eobrun_at_scan_end for c in eo if f"limit{limit}_" in c[0]), limit
    assert big.eobrun_at_scan_end and any(c[2].eobrun_flushed_at_restart for c in eo)
    assert {len(tab.syms) == 1 or min(tab.lengths().values()) == 16 for c in eo if "all16" in c[0] for tab in c[2].tables.values()} == {True}
    census = sum((c[2].census for c in family("prog_tables")), Counter())
    for dcs, acs, _ in SHAPES:                                      # every shape but the one-symbol tables and the ladder from 1 bit: a scan's
        if "single" not in dcs + acs and "ladder1" not in dcs + acs:   # band decides its symbols (eobruns_ has such tables, scan by scan)
            assert census["dc_" + dcs] and census["ac_" + acs], (dcs, acs)
    assert len({c[0] for c in valid()}) == len(valid())
    return {name: len(family(name)) for name in FAMILIES}


# ---- T: tolerated streams ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tolerated():
    cases = []
    w, h = 40, 24
    comps = components("gray")
    tabs = shaper("random2", "random2", 600)

    def blocks(**kw):
        coefs = coefficients(np.random.default_rng(20), w, h, comps)
        return W.write(w, h, comps, coefs, steps(2), tabs, **kw)[0]

    dc0 = [("s", 0, 0)]
    cases.append(("tolerated_run_passes_63", blocks(override={(0, 1, 2): dc0 + [("s", 1, 0x31), ("b", 1, 1), ("s", 1, 0xF0), ("s", 1, 0xF0), ("s", 1, 0xF0), ("s", 1, 0xE2), ("b", 3, 2), ("s", 1, 0x00)]}),
                  2, "ke_jpeg_core.h ke_decode_block: k > 63 behind a run (libjpeg stores nothing there and reads on)"))
    cases.append(("tolerated_zrl_chain_reaches_64_then_eob", blocks(override={(0, 1, 2): dc0 + [("s", 1, 0xF0)] * 4 + [("s", 1, 0x00)]}),
                  2, "ke_jpeg_core.h ke_decode_block: the stray EOB is read as the next block's DC code and the stream is misread from there on"))
    cases.append(("tolerated_zrl_chain_reaches_64_then_eob_last_block", blocks(override={(0, 2, 4): dc0 + [("s", 1, 0xF0)] * 4 + [("s", 1, 0x00)]}),
                  0, "the stray EOB lies behind the last block: nobody reads it"))
    for cat in (12, 13, 14, 15):
        cases.append((f"tolerated_dc_category_{cat}", blocks(override={(0, 1, 1): [("s", 0, cat), ("b", 1 << (cat - 1), cat), ("s", 1, 0x00)]}),
                      2, "ke_jpeg_core.h ke_decode_block: s > 11 (a DC difference of 8-bit samples has 11 bits at most)"))
    cases.append(("tolerated_fill_bytes_in_front_of_a_restart_marker", blocks(restart=4, before_marker={1: b"\xff"}),
                  1, "ke_jpeg_parse.h ke_jpeg_segment_end: FF FF ends the entropy data, and what ends it must be the EOI"))
    cases.append(("tolerated_fill_bytes_in_front_of_the_eoi", blocks(before_marker={"eoi": b"\xff\xff"}),
                  1, "ke_jpeg_parse.h ke_jpeg_segment_end: the first FF not followed by 00 or RSTn must be the EOI's"))
    cases.append(("tolerated_restart_marker_with_the_wrong_number", blocks(restart=3, rst_number=lambda k: k + (k >= 2)),
                  2, "ke_jpeg_core.h ke_bits_restart: marker != RST(next_rst) (libjpeg resynchronises by a heuristic)"))
    cases.append(("tolerated_data_ends_three_mcus_early", blocks(stop_after=12),
                  2, "ke_jpeg_core.h ke_bits_ran_dry: bits used that are not in the file (libjpeg feeds zeros, with a warning)"))
    cases.append(("tolerated_data_ends_early_restarts", blocks(restart=5, stop_after=13),
                  2, "ke_jpeg_core.h ke_bits_restart: no marker where the next interval should begin"))
    # a scan that names a table no DHT defines: libjpeg-turbo then installs the standard tables of Annex K (jinit_huff_decoder does it
    # for Motion JPEG frames) and decodes, whatever the data was coded with
    cases.append(("tolerated_scan_names_a_table_never_defined", _undefined_table(), 2, "ke_jpeg_parse.h ke_parse_jpeg, SOS: ac_tab[ta] < 0 (the standard tables are not assumed)"))
    return tuple(cases)


def _undefined_table():
    w, h = 24, 16
    comps = components("444")
    good = {}

    def remember(si, cls, tid, counter):
        good[(cls, tid)] = shaper("ladder2", "random3", 700)(si, cls, tid, counter)
        return good[(cls, tid)]

    coefs = coefficients(np.random.default_rng(21), w, h, comps)
    W.write(w, h, comps, coefs, steps(1, 1), remember)
    raw = [W.segment(0xC4, bytes([(c << 4) | t]) + good[(c, t)].payload) for (c, t) in sorted(good) if (c, t) != (1, 1)]
    return W.write(w, h, comps, coefs, steps(1, 1), good, raw_dht=raw)[0]


# ---- R: refused tables -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refused():
    cases = []
    w, h = 24, 16
    comps = components("444", td=(0, 1, 1), ta=(0, 1, 1))
    coefs = coefficients(np.random.default_rng(21), w, h, comps)
    good = {}

    def remember(si, cls, tid, counter):
        good[(cls, tid)] = shaper("ladder2", "random3", 700)(si, cls, tid, counter)
        return good[(cls, tid)]

    W.write(w, h, comps, coefs, steps(1, 1), remember)

    def dht(key, counts, syms):
        return W.segment(0xC4, bytes([(key[0] << 4) | key[1]]) + bytes(counts) + bytes(syms))

    def file(**replace):
        raw = [replace.get(f"t{c}{t}", dht((c, t), good[(c, t)].counts, good[(c, t)].syms)) for (c, t) in sorted(good)]
        return W.write(w, h, comps, coefs, steps(1, 1), good, raw_dht=[r for r in raw if r])[0]

    t = good[(0, 1)]
    cases.append(("refused_dc_symbol_above_15", file(t01=dht((0, 1), t.counts, t.syms[:-1] + [16]))))
    cases.append(("refused_all_ones_code_of_2_bits_in_use", file(t10=dht((1, 0), [1, 2] + [0] * 14, [0x00, 0x01, 0x02]))))      # 0 | 10, 11
    cases.append(("refused_all_ones_code_of_16_bits_in_use", file(t10=dht((1, 0), [1] * 15 + [2], list(range(17))))))         # ... | 1..10, 1..11
    cases.append(("refused_counts_overflow_a_length", file(t10=dht((1, 0), [3] + [0] * 15, [0x00, 0x01, 0x02]))))              # three codes of one bit
    seg = dht((1, 1), good[(1, 1)].counts, good[(1, 1)].syms)
    cases.append(("refused_dht_segment_longer_than_its_table", file(t11=seg[:2] + (len(seg) - 2 + 3).to_bytes(2, "big") + seg[4:] + b"\x00\x00\x00")))
    return tuple(cases)
