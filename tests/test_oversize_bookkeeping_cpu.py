"""The oversize route's bookkeeping without a GPU: refine._decode_on_gpu over a context whose decode calls answer with arrays
written here, at the real max_side of 4096, where the window of formats.seam_actions is not empty -- which files are counted
as ``gpu_oversize`` (shrunk from beyond the window, or drafted into it), which call each file goes to, and the bounds beyond
which formats.seam_actions leaves a file to the loader instead of sending it to a kernel that would refuse it."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

M = 4096
# name: (file's width, height, channels, status, orientation or 0 for none), what becomes of it with the variable set:
# (the drafted size, the action's name, counted as gpu_oversize)
JPEG = {
    "small.jpg": ((3000, 2000, 3, 0, 0), ((3000, 2000), "as_decoded", False)),
    "window.jpg": ((6000, 4000, 3, 0, 0), ((6000, 4000), "shrink", False)),
    "camera_108mp.jpg": ((12000, 9000, 3, 0, 0), ((6000, 4500), "shrink", True)),          # 1/2, into the old window
    "camera_turned.jpg": ((12000, 9000, 3, 0, 6), ((6000, 4500), "turn_shrink", True)),
    "drafted_fits.jpg": ((8192, 8192, 3, 0, 0), ((4096, 4096), "as_decoded", True)),       # 1/2, nothing left to shrink
    "drafted_window_turned.jpg": ((8200, 8192, 3, 0, 3), ((4100, 4096), "turn_shrink", True)),
    "drafted_normalise.jpg": ((8192, 8192, 3, 0, 8), ((4096, 4096), "normalise", True)),
    "panorama.jpg": ((16000, 2600, 3, 0, 0), ((16000, 2600), "oversize", True)),           # the short side keeps it at 1/1
    "huge.jpg": ((32000, 8200, 3, 0, 0), ((16000, 4100), "oversize", True)),               # 1/2, still past the window
    "huge_turned.jpg": ((8200, 32000, 3, 0, 6), ((4100, 16000), "oversize", True)),
    "gray.jpg": ((12000, 9000, 1, 0, 0), ((6000, 4500), "leave", False)),
    "handed_back.jpg": ((12000, 9000, 3, 1, 0), ((6000, 4500), "leave", False)),
}
PNG = {
    "scan.png": ((9921, 7016, 3, 0, 0), ((9921, 7016), "oversize", True)),
    "rgba.png": ((9921, 7016, 4, 0, 0), ((9921, 7016), "leave", False)),
    "page.png": ((2000, 3000, 3, 0, 0), ((2000, 3000), "as_decoded", False)),
}


class Context:
    """decode_files_owned answers from the tables above (JPEG files at the draft scale when asked); every other call records
    what it was given and hands out a fresh address."""

    def __init__(self):
        self.calls, self.next = [], 1 << 20

    def _address(self):
        self.next += 1 << 20
        return self.next

    def decode_files_owned(self, paths, kind, draft_side=None):
        from kobato_eyes_amd import _native

        table = JPEG if kind == "jpeg" else PNG
        w, h, c, st, o = (np.array(col, np.int32) for col in zip(*(table[os.path.basename(p)][0] for p in paths)))
        flags = np.where(o > 0, 1 | (o << 8), 0).astype(np.int32)
        off = (np.arange(len(paths)) * 64).astype(np.uint64)
        self.calls.append(("decode", kind, draft_side))
        if draft_side is None:
            return self._address(), off, w, h, c, st, flags
        d = _native.draft_scale(w, h, draft_side)
        return self._address(), off, -(-w // d), -(-h // d), c, st, flags, d

    def normalise_rgb(self, dev, off, w, h, c, orient):
        self.calls.append(("normalise", [(int(a), int(b), int(o)) for a, b, o in zip(w, h, orient)]))
        turned = np.asarray(orient) >= 5
        return self._address(), (np.arange(len(w)) * 64).astype(np.uint64), np.where(turned, h, w), np.where(turned, w, h)

    def thumbnail_rgb(self, addr, w, h, box):
        from kobato_eyes_amd import _native

        self.calls.append(("thumbnail", w, h, box))
        return (self._address(),) + tuple(_native.thumbnail_size(w, h, box))

    def thumbnail_rgb_reduced(self, addr, w, h, box):
        from kobato_eyes_amd import _native

        self.calls.append(("reduced", w, h, box))
        x, y = _native.thumbnail_size(w, h, box)
        return self._address(), x, y, (int(w / x / 2.0) or 1, int(h / y / 2.0) or 1)

    def free(self, dev):
        self.calls.append(("free", dev))


def run(monkeypatch, variable):
    from kobato_eyes_amd import refine

    for name in ("KE_GPU_REFINE_DECODE", "KE_GPU_JPEG", "KE_GPU_PNG"):
        monkeypatch.delenv(name, raising=False)
    if variable is None:
        monkeypatch.delenv("KE_GPU_REFINE_OVERSIZE", raising=False)
    else:
        monkeypatch.setenv("KE_GPU_REFINE_OVERSIZE", variable)
    ctx, placed, buffers = Context(), {}, []
    count = {"decodes": 0, "gpu_decodes": 0, "fit_launches": 0, "ssim_launches": 0, "pairs": 0}
    need = ["/pictures/" + n for n in list(JPEG) + list(PNG)]
    refine._decode_on_gpu(ctx, need, placed, buffers, count, M)
    return ctx, placed, count


def test_with_the_variable_set_every_file_kept_from_the_loader_is_counted_once(monkeypatch):
    from kobato_eyes_amd import _native

    ctx, placed, count = run(monkeypatch, "1")
    expected = {**JPEG, **PNG}
    assert ("decode", "jpeg", M) in ctx.calls and ("decode", "png", None) in ctx.calls
    stay = {n for n, (_, (_, action, _)) in expected.items() if action != "leave"}
    assert {os.path.basename(p) for p in placed} == stay
    for n in stay:
        (_, _, _, _, o), ((w, h), action, _) = expected[n]
        if o >= 5:
            w, h = h, w
        size = (w, h) if max(w, h) <= M else _native.thumbnail_size(w, h, M)
        assert placed["/pictures/" + n][1:] == size, n
    assert count["gpu_oversize"] == sum(counted for _, (_, _, counted) in expected.values()) == 9
    assert count["gpu_decodes"] == len(stay)
    # the calls: files past the window go through the reduce route at their drafted (and turned) sizes, those drafted into the
    # window through the plain shrink
    assert sorted(c[1:3] for c in ctx.calls if c[0] == "reduced") == sorted([(16000, 2600), (16000, 4100), (16000, 4100), (9921, 7016)])
    assert sorted(c[1:3] for c in ctx.calls if c[0] == "thumbnail") == sorted([(6000, 4000), (6000, 4500), (4500, 6000), (4100, 4096)])
    assert all(c[3] == M for c in ctx.calls if c[0] in ("reduced", "thumbnail"))
    assert count["gpu_shrunk"] == 4 and count["gpu_normalised"] == 1


def test_with_the_variable_unset_nothing_is_drafted_or_counted(monkeypatch):
    for variable in (None, "0"):
        ctx, placed, count = run(monkeypatch, variable)
        assert ("decode", "jpeg", M) not in ctx.calls and not any(c[0] == "reduced" for c in ctx.calls)
        assert "gpu_oversize" not in count
        assert {os.path.basename(p) for p in placed} == {"small.jpg", "window.jpg", "page.png"}


def test_a_file_that_fits_is_never_shrunk_whatever_max_side():
    """Below max_side = 256 the old window is empty; the oversize action starts behind the files that fit, not on them."""
    from kobato_eyes_amd import formats as F

    w, h = np.array([64, 50, 65, 7, 200], np.int32), np.array([64, 40, 3, 64, 130], np.int32)
    c, st, flags = np.full(5, 3, np.int32), np.zeros(5, np.int32), np.zeros(5, np.int32)
    for kind in ("jpeg", "png"):
        actions, _ = F.seam_actions(kind, "refine", w, h, c, st, flags, 64, oversize=True)
        assert actions.tolist() == [F.AS_DECODED, F.AS_DECODED, F.SHRINK_OVERSIZE, F.AS_DECODED, F.SHRINK_OVERSIZE]


@pytest.mark.parametrize("m", [64, 4096])
def test_what_the_kernels_would_refuse_stays_with_the_loader(m):
    """ke_reduce_rgb takes factors up to 255 and the resampler writes at most 4096 samples a side: formats.seam_actions answers
    SHRINK_OVERSIZE only where neither is passed -- every factor of every file it sends is computed here."""
    from kobato_eyes_amd import _native
    from kobato_eyes_amd import formats as F

    rng = np.random.default_rng(5)
    # random sizes, the sizes about the bounds, and the longest side that is sent against every short side whose target is a
    # few samples (where the whole-number target is furthest below the side's share)
    edge = np.arange(1, 800)
    longer = np.concatenate([rng.integers(m + 1, 600 * m, 400), [F.OVERSIZE_MAX_RATIO * m, F.OVERSIZE_MAX_RATIO * m + 1, 512 * m, 513 * m],
                             np.full(len(edge), F.OVERSIZE_MAX_RATIO * m)])
    shorter = np.minimum(np.concatenate([rng.integers(1, 3 * m, 200), rng.integers(1, 12, 204), edge]), F.OVERSIZE_MAX_PIXELS // longer)
    swap = rng.integers(0, 2, len(longer)).astype(bool)
    w, h = np.where(swap, shorter, longer).astype(np.int32), np.where(swap, longer, shorter).astype(np.int32)
    n = len(w)
    actions, _ = F.seam_actions("png", "refine", w, h, np.full(n, 3, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), m, oversize=True)
    sent = np.nonzero(actions == F.SHRINK_OVERSIZE)[0]
    assert 0 < len(sent) < n and (actions[longer > F.OVERSIZE_MAX_RATIO * m] == F.LEAVE).all()
    assert (actions[(longer <= F.OVERSIZE_MAX_RATIO * m) & (longer >= 2 * m)] == F.SHRINK_OVERSIZE).all()
    worst = 0
    for k in sent.tolist():
        x, y = _native.thumbnail_size(int(w[k]), int(h[k]), m)
        worst = max(worst, int(w[k] / x / 2.0), int(h[k] / y / 2.0))
        assert max(x, y) <= 4096
    print("largest factor sent:", worst)
    assert 128 < worst <= 255
    # the long strip of 40 x 2.1 M pixels, a PNG file the decoder takes: its factor would be 256
    strip = F.seam_actions("png", "refine", np.array([40], np.int32), np.array([2_100_000], np.int32), np.array([3], np.int32),
                           np.zeros(1, np.int32), np.zeros(1, np.int32), 4096, oversize=True)[0]
    assert strip.tolist() == [F.LEAVE] and int(2_100_000 / 4096 / 2.0) > 255
    over = F.seam_actions("png", "refine", np.array([20000], np.int32), np.array([9000], np.int32), np.array([3], np.int32),
                          np.zeros(1, np.int32), np.zeros(1, np.int32), 8192, oversize=True)[0]
    assert over.tolist() == [F.LEAVE]
