"""A progressive JPEG writer for the decoder tests: quantised coefficients in, a file with ANY legal scan script out.  Pillow's
writer (libjpeg-turbo) only ever produces libjpeg's default script; files from other encoders (mozjpeg: what most image hosts
serve) order and split their scans differently -- DC scans for one, two or all components, spectral bands cut anywhere,
successive approximation from any bit down -- and the decoder has to be held against Pillow on those too.  The entropy coding
is tests/_jpeg_write.py's (T.81 Annex G as libjpeg's jcphuff.c does it); as called here it writes one end-of-band symbol per
block, no end-of-band runs and no restarts, with the standard Huffman tables of Annex K, taken from a file Pillow writes."""
from __future__ import annotations

import io
import struct

import numpy as np
from PIL import Image

import _jpeg_write as W


def _standard_tables():
    """{(class, id): {symbol: (code, length)}} from the DHT segments of a baseline file Pillow writes without optimisation."""
    b = io.BytesIO()
    Image.fromarray(np.zeros((16, 16, 3), np.uint8)).save(b, "JPEG", quality=75)
    data = b.getvalue()
    tables, raw = {}, {}
    pos = 2
    while pos < len(data) and data[pos] == 0xFF and data[pos + 1] != 0xDA:
        marker, n = data[pos + 1], struct.unpack(">H", data[pos + 2:pos + 4])[0]
        if marker == 0xC4:
            at, end = pos + 4, pos + 2 + n
            while at < end:
                tc_th = data[at]
                counts = list(data[at + 1:at + 17])
                syms = list(data[at + 17:at + 17 + sum(counts)])
                raw[(tc_th >> 4, tc_th & 15)] = bytes(data[at:at + 17 + sum(counts)])
                code, k, table = 0, 0, {}
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        table[syms[k]] = (code, length)
                        code += 1
                        k += 1
                    code <<= 1
                tables[(tc_th >> 4, tc_th & 15)] = table
                at += 17 + sum(counts)
        pos += 2 + n
    return tables, raw


_TABLES, _RAW = _standard_tables()


def encode(width: int, height: int, comps, coefs, script, qtables=None, tables=None, **options) -> bytes:
    """comps: [(id, hs, vs)]; coefs[c]: int array [padded block rows][padded block columns][64] in zigzag order (padded to whole
    MCUs); script: [(component indices, ss, se, ah, al)] -- any order T.81 allows.  tables: what tests/_jpeg_write.py's `write`
    takes as `htables` instead of the standard pair; options: its other keywords (restart intervals, end-of-band runs, ...)."""
    qtables = qtables or [np.ones(64, np.uint8), np.ones(64, np.uint8)]
    standard = {key: W.Table(raw[1:17], raw[17:]) for key, raw in _RAW.items() if key[1] == 0}
    full = [(cid, hs, vs, 0 if k == 0 else 1, 0, 0) for k, (cid, hs, vs) in enumerate(comps)]
    return W.write(width, height, full, coefs, qtables, tables or standard, sof=0xC2, script=script, **options)[0]


def random_script(rng, ncomp: int):
    """A random legal progression: DC scans for all, some or single components from a random bit down; for every component its
    AC coefficients cut into 1..4 bands, each from a random bit down; scans shuffled as far as the rules allow (a component's
    first DC scan before its AC scans, a band's refinements in order)."""
    chains = []
    al0 = int(rng.integers(0, 3))
    groups = [list(range(ncomp))] if ncomp == 1 or rng.integers(0, 2) else ([[0], list(range(1, ncomp))] if rng.integers(0, 2) else [[c] for c in range(ncomp)])
    dc_first = [(g, 0, 0, 0, al0) for g in groups]
    for bit in range(al0, 0, -1):
        g2 = [list(range(ncomp))] if rng.integers(0, 2) else [[c] for c in range(ncomp)]
        chains.append([(g, 0, 0, bit, bit - 1) for g in g2])
    # refinements of DC must follow each other in order: one chain
    dc_chain = [s for level in chains for s in level]
    chains = [dc_chain] if dc_chain else []
    for c in range(ncomp):
        cuts = sorted(set(rng.integers(2, 64, int(rng.integers(0, 4))).tolist()))
        edges = [1] + cuts + [64]
        for lo, hi in zip(edges[:-1], edges[1:]):
            al = int(rng.integers(0, 3))
            chain = [([c], lo, hi - 1, 0, al)] + [([c], lo, hi - 1, bit, bit - 1) for bit in range(al, 0, -1)]
            chains.append(chain)
    script = list(dc_first)
    rng.shuffle(script)
    heads = [0] * len(chains)
    while any(h < len(ch) for h, ch in zip(heads, chains)):
        k = int(rng.choice([i for i, (h, ch) in enumerate(zip(heads, chains)) if h < len(ch)]))
        script.append(chains[k][heads[k]])
        heads[k] += 1
    return script


def random_file(rng, width: int, height: int, sampling: str = "444", gray: bool = False):
    """(file bytes, script) for random smooth-ish coefficients."""
    comps = [(1, 1, 1)] if gray else [(1, {"444": 1, "422": 2, "420": 2, "440": 1}[sampling], {"444": 1, "422": 1, "420": 2, "440": 2}[sampling]), (2, 1, 1), (3, 1, 1)]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mcus_x, mcus_y = -(-width // (8 * hmax)), -(-height // (8 * vmax))
    coefs = []
    for (_, hs, vs) in comps:
        shape = (mcus_y * vs, mcus_x * hs, 64)
        a = np.zeros(shape, np.int32)
        a[:, :, 0] = rng.integers(-60, 61, shape[:2]) * 8
        decay = np.maximum(1, (40 / (1 + np.arange(64))).astype(np.int32))
        a[:, :, 1:] = (rng.integers(-1, 2, (shape[0], shape[1], 63)) * rng.integers(0, decay[1:] + 1, (shape[0], shape[1], 63))) * (rng.random((shape[0], shape[1], 63)) < 0.35)
        coefs.append(a)
    q = [np.full(64, 2, np.uint8), np.full(64, 3, np.uint8)]
    script = random_script(rng, len(comps))
    return encode(width, height, comps, coefs, script, q), script
