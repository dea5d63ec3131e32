"""ke_webpn_decode on the GPU: the first frame of animated WebP files against Pillow, bit for bit -- every valid case in one
shuffled batch with the refused ones interleaved, canvases at every alignment with guard bytes behind each; the probe's shapes;
the hashes against the oracle's of Pillow's pixels; a bounded damage sample; the same batch in sub-batches; the batch hasher with
KE_GPU_WEBP_ANIMATED set and unset.  Small shapes only: no canvas here is over 300 x 300."""
from __future__ import annotations

import numpy as np
import pytest

import _webp_cases as W
import _webpa_cases as A
import _webpl_cases as L
import _webpn_cases as N
from oracle import oracle as O

pytestmark = pytest.mark.gpu
GUARD = 32


def _native():
    from kobato_eyes_amd import _native

    return _native


@pytest.fixture(scope="module")
def ctx():
    return _native().get_context(0)


@pytest.fixture(scope="module")
def batch():
    """[(name, file, expected status, Pillow's pixels or None)]: the valid cases with the invalid and the unshared ones in
    between, shuffled; Pillow's pixels computed once."""
    refused = [(n, d, e) for n, d, e in N.invalid_cases()] + [(n, d, N.UNSUPPORTED) for n, d in N.unshared_cases() if n != "canvas_over_cap"]
    out = []
    for k, (_, name, data) in enumerate(N.valid_cases()):
        out.append((name, data, N.OK, N.pillow_pixels(data)))
        if k % 5 == 4:
            out.append(refused[(k // 5) % len(refused)] + (None,))
    out += [r + (None,) for r in refused]
    order = np.random.default_rng(42).permutation(len(out))
    return [out[k] for k in order.tolist()]


def _decode_with_guards(ctx, blobs):
    """ke_webpn_decode into a buffer of its own whose canvases lie at every alignment with GUARD bytes of 0xA5 behind each (a
    refused file has the guard alone): the per-file status, the canvases and the guards as the call left them."""
    K = _native()
    with ctx._lock:
        files = ctx._packed(blobs)
        w, h, c, st = ctx._probe(files, "webpn")
        nbytes = np.where(st == 0, w.astype(np.int64) * h * c, 0)
        off = np.zeros(len(blobs), np.uint64)
        at = 0
        for k, nb in enumerate(nbytes.tolist()):
            off[k] = at
            at += nb + GUARD + k % 7                                   # canvases start at every alignment
        host = np.full(at + 64, 0xA5, np.uint8)
        dev = ctx.malloc(host.nbytes)
        try:
            ctx.memcpy(dev, host, host.nbytes)
            ctx._check(ctx._lib.ke_webpn_decode(ctx._h, K._addr(files.flat), K._addr(files.offsets), K._addr(files.sizes), len(blobs), dev,
                                                K._addr(off), K._addr(st)), "ke_webpn_decode")
            sub_batches = ctx.last_decode_sub_batches()
            ctx.memcpy(host, dev, host.nbytes)
        finally:
            ctx.free(dev)
    canvases, guards = [], []
    for k, nb in enumerate(nbytes.tolist()):
        o = int(off[k])
        canvases.append(host[o:o + nb].reshape(int(h[k]), int(w[k]), int(c[k])) if nb else None)
        guards.append(host[o + nb:o + nb + GUARD])
    return st, canvases, guards, sub_batches


def _hold(batch, st, canvases, guards):
    alignments = set()
    for (name, data, expected, ref), s, px, guard in zip(batch, st.tolist(), canvases, guards):
        assert s == expected, (name, s, expected)
        assert (guard == 0xA5).all(), f"{name}: bytes behind the canvas, or a refused file's slot, were written"
        if s == N.OK:
            assert px.shape == ref.shape, (name, px.shape, ref.shape)
            assert np.array_equal(px, ref), name
            alignments.add((px.shape[2], px.ctypes.data % 4 == 0))
    return alignments


def test_webpn_decode_matches_pillow_in_one_shuffled_batch(ctx, batch):
    """Status and pixels equal Pillow's, guard bytes hold, a refused file's slot is untouched; three and four channels both went
    through the dword stores and the byte stores."""
    st, canvases, guards, sub_batches = _decode_with_guards(ctx, [d for _, d, _, _ in batch])
    assert _hold(batch, st, canvases, guards) == {(3, False), (3, True), (4, False), (4, True)}
    assert sub_batches == 1 and (st == 0).sum() == len(N.valid_cases()) and (st != 0).sum() > 60


def test_webpn_sub_batches_give_the_same(ctx, batch, monkeypatch):
    """A scratch budget of 256 KiB cuts the batch into many sub-batches, mixed ones among them: identical results."""
    monkeypatch.setenv("KE_WEBP_SCRATCH_BYTES", str(256 << 10))
    st, canvases, guards, sub_batches = _decode_with_guards(ctx, [d for _, d, _, _ in batch])
    _hold(batch, st, canvases, guards)
    assert sub_batches > 3, sub_batches


def test_webpn_probe_and_the_context_calls(ctx, batch):
    """Probe shapes equal Pillow's; Context.webpn_decode hands the same canvases back."""
    some = batch[:120]
    w, h, c, st = ctx.webpn_probe([d for _, d, _, _ in some])
    out, status = ctx.webpn_decode([d for _, d, _, _ in some])
    for k, (name, data, expected, ref) in enumerate(some):
        assert status[k] == expected, (name, status[k])
        if expected == N.OK:
            assert st[k] == 0 and (h[k], w[k], c[k]) == ref.shape, name
            assert np.array_equal(out[k], ref), name
        else:
            assert out[k] is None, name


def test_webpn_hash_equals_the_oracle_of_pillow_pixels(ctx, batch):
    cases = [(n, d, ref) for n, d, e, ref in batch if e == N.OK and min(ref.shape[:2]) >= 8]
    ph, dh, st = ctx.webpn_hash([d for _, d, _ in cases])
    for k, (name, data, ref) in enumerate(cases):
        assert st[k] == 0 and (int(ph[k]), int(dh[k])) == O.hash_image(ref), name
    assert len(cases) > 150


def test_webpn_damage_is_refused_or_equal_to_pillow(ctx):
    """A bounded sample of the CPU test's damage through the kernels, with its rules: Pillow still opens at least a quarter of the
    files, and the decoder takes at least three quarters of those (the CPU build's first run: 87 %; the first run here: 330 of 377)."""
    damaged = N.byte_changes(600, seed=114) + N.cut_cases()[::9]
    out, status = ctx.webpn_decode([d for _, d in damaged])
    taken = pillow_ok = 0
    for (name, data), px, st in zip(damaged, out, status):
        assert st in (N.OK, N.UNSUPPORTED, N.CORRUPT), name
        ref = N.pillow_pixels(data)
        pillow_ok += ref is not None
        if st == N.OK:
            taken += 1
            assert ref is not None and px.shape == ref.shape and np.array_equal(ref, px), name
    print(f"damage on the GPU: {len(damaged)} files, Pillow opens {pillow_ok}, the decoder takes {taken}")
    assert len(damaged) >= 700 and 4 * pillow_ok >= len(damaged) and 4 * taken >= 3 * pillow_ok


def test_batch_hasher_rows_with_the_animated_route_on_and_off(tmp_path, monkeypatch):
    """Animated and still .webp files in one directory: the Pillow route's rows with KE_GPU_WEBP_ANIMATED=1 as without it, and
    the animated files reach the Pillow share only when it is unset."""
    from kobato_eyes_amd import fastsig as K

    big = lambda d: min(N.pillow_pixels(d).shape[:2]) >= 8              # noqa: E731
    animated = [(n, d) for f, n, d in N.valid_cases() if f in ("codec_flag", "placed", "frames", "pillow", "meta") and big(d)][:90]
    lossy = [c for c in W.taken_cases()[:40] if min(W.pillow_rgb(c[1]).shape[:2]) >= 8][:20]
    alpha = [(n, d) for _, n, d in A.all_taken(None)[:40] if big(d)][:15]
    lossless = [c for c in L.taken_cases()[:40] if big(c[1])][:15]
    others = [(n, d) for n, d in N.unshared_cases() if n in ("empty_anmf", "later_anmf_size_differs")]       # Pillow's either way
    items = []
    for k, (_, data) in enumerate(animated + lossy + alpha + lossless + others):
        p = tmp_path / f"{k:03d}.webp"
        p.write_bytes(data)
        items.append((900 + k, str(p)))
    seen = []
    original = K._Pipeline._decode_with_pillow

    def spy(self, todo, out):
        seen.extend(self.paths[k] for k in todo)
        return original(self, todo, out)

    monkeypatch.setattr(K._Pipeline, "_decode_with_pillow", spy)
    fill = lambda todo: K.fast_fill_missing_signatures("", todo, max_workers=4, chunksize=16, apply_to_db=False)      # noqa: E731
    for v in ("KE_GPU_WEBP_LOSSLESS", "KE_GPU_WEBP_ALPHA", "KE_GPU_WEBP_ANIMATED"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("KE_GPU_WEBP", "0")                                   # every file through Pillow: the rows to equal
    want = fill(items)
    assert len(want) == len(items)
    monkeypatch.delenv("KE_GPU_WEBP")
    animated_paths = {p for _, p in items[:len(animated)]}
    other_paths = {p for _, p in items[-len(others):]}
    seen.clear()
    assert fill(items) == want
    assert animated_paths | other_paths <= set(seen)                         # the variable unset: as before
    monkeypatch.setenv("KE_GPU_WEBP_ANIMATED", "1")
    seen.clear()
    assert fill(items) == want
    assert not animated_paths & set(seen), "an animated file went to the Pillow share"
    assert other_paths <= set(seen)
    monkeypatch.setenv("KE_GPU_WEBP_LOSSLESS", "1")                          # beside the other follow-ups of webp
    monkeypatch.setenv("KE_GPU_WEBP_ALPHA", "1")
    seen.clear()
    assert fill(items) == want
    assert not animated_paths & set(seen) and other_paths <= set(seen)
    monkeypatch.setenv("KE_GPU_WEBP", "0")                                   # the whole WebP route off: the variable alone does nothing
    seen.clear()
    assert fill(items) == want
    assert animated_paths <= set(seen)
