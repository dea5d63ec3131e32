"""_views.view_signatures -- the one path behind turned_signatures, trimmed_signatures and turned_trimmed_signatures -- without a
GPU: a stub context stands for the decoders and the hash calls, and formats.enabled_kinds is cut to two kinds, so that the loop
itself is what runs: which files a call is offered, where its rows land, what falls to Pillow and what a file nobody opens
leaves behind.

The stub's answer for a file is made from one number: the file's stem for a device call, the picture's first pixel plus 1000 for
a call on pictures Pillow opened, so a row says which route made it."""
from __future__ import annotations

import numpy as np
import pytest
from PIL import Image

from kobato_eyes_amd import _native, _views, formats, trimmed, turned, turned_trimmed

# what the public functions document: the arrays before ``ok``, as (trailing shape, dtype)
DOCUMENTED = {
    "turned": [((8,), np.uint64)],
    "trimmed": [((), np.uint64), ((4,), np.int32), ((), np.bool_)],
    "turned_trimmed": [((8,), np.uint64), ((8,), np.uint64), ((4,), np.int32), ((), np.bool_)],
}
PUBLIC = {"turned": turned.turned_signatures, "trimmed": trimmed.trimmed_signatures, "turned_trimmed": turned_trimmed.turned_trimmed_signatures}


def _answer(mode, numbers):
    """The stub's outputs for files of these numbers: output j of number v holds v + 100 j throughout (a flag: v is odd)."""
    v = np.asarray(numbers, np.int64)
    return [(v % 2 == 1) if dtype is np.bool_ else (np.broadcast_to((v + 100 * j).reshape((-1,) + (1,) * len(shape)), (len(v),) + shape).astype(dtype))
            for j, (shape, dtype) in enumerate(DOCUMENTED[mode])]


class _Context:
    def __init__(self, mode, refused=()):
        self.mode, self.refused, self.on_device, self.on_host = mode, set(refused), [], []
        on_device, on_host, _ = _views.CALLS[mode]
        setattr(self, on_device, self._device_call)
        setattr(self, on_host, self._host_call)

    def _device_call(self, blobs, *, kind, paths, **keywords):
        assert blobs is None
        self.on_device.append((kind, list(paths), keywords))
        numbers = [int(p.rsplit("/", 1)[1].split(".")[0]) for p in paths]
        status = np.array([1 if n in self.refused else 0 for n in numbers], np.int32)
        return (*[a * (status == 0).reshape((-1,) + (1,) * (a.ndim - 1)) for a in _answer(self.mode, numbers)], status)

    def _host_call(self, images, **keywords):
        self.on_host.append(([im.shape for im in images], keywords))
        assert len({im.ndim for im in images}) == 1
        return (*_answer(self.mode, [1000 + int(im.reshape(-1)[0]) for im in images]), np.zeros(len(images), np.int32))


@pytest.fixture
def files(tmp_path, monkeypatch):
    """1.png grey, 2.png and 128.jpg RGB, 4.png grey, 5.png not a picture; every pixel of a picture is its number."""
    monkeypatch.setattr(formats, "enabled_kinds", lambda seam: [("jpeg", (".jpg",)), ("png", (".png",))])
    for name, shape in (("1.png", (5, 7)), ("2.png", (4, 6, 3)), ("128.jpg", (8, 8, 3)), ("4.png", (3, 3))):
        Image.fromarray(np.full(shape, int(name.split(".")[0]), np.uint8)).save(tmp_path / name)
    (tmp_path / "5.png").write_bytes(b"not a picture")
    return {int(name.split(".")[0]): str(tmp_path / name) for name in ("1.png", "2.png", "128.jpg", "4.png", "5.png")}


def _use(monkeypatch, ctx):
    monkeypatch.setattr(_native, "get_context", lambda device=0, role="": ctx)
    return ctx


@pytest.mark.parametrize("mode", list(DOCUMENTED))
def test_two_equal_paths_get_one_decode_and_two_rows(monkeypatch, files, mode):
    ctx = _use(monkeypatch, _Context(mode))
    *got, ok = _views.view_signatures(mode, [files[1], files[128], files[1], files[2]], 31, 0)
    keywords = {} if mode == "turned" else {"tolerance": 31}
    assert ctx.on_device == [("jpeg", [files[128]], keywords), ("png", [files[1], files[2]], keywords)] and ctx.on_host == []
    assert ok.tolist() == [True] * 4
    for mine, want in zip(got, _answer(mode, [1, 128, 1, 2])):
        assert mine.dtype == want.dtype and np.array_equal(mine, want)


@pytest.mark.parametrize("mode", list(DOCUMENTED))
def test_a_refused_file_falls_to_pillow_and_an_unreadable_one_has_zeros(monkeypatch, files, mode):
    ctx = _use(monkeypatch, _Context(mode, refused=(1, 128, 4, 5)))
    order = [5, 1, 2, 128, 4]
    *got, ok = _views.view_signatures(mode, [files[n] for n in order], 31, 0)
    keywords = {} if mode == "turned" else {"tolerance": 31}
    assert [(kind, len(paths)) for kind, paths, _ in ctx.on_device] == [("jpeg", 1), ("png", 4)]
    # what the decoders left, by channel count: the two grey pictures in one call, the JPEG in another; 5.png reaches neither
    assert sorted(ctx.on_host, key=lambda c: len(c[0])) == [([(8, 8, 3)], keywords), ([(5, 7), (3, 3)], keywords)]
    assert ok.tolist() == [False, True, True, True, True]
    want = _answer(mode, [0, 1001, 2, 1128, 1004])
    for mine, expected in zip(got, want):
        expected = expected.copy()
        expected[0] = 0                                                     # nobody opened it: zeros, flag False
        assert np.array_equal(mine, expected), (mine, expected)


@pytest.mark.parametrize("n", [0, 3])
@pytest.mark.parametrize("mode", list(DOCUMENTED))
def test_every_mode_returns_the_documented_arrays(monkeypatch, files, mode, n):
    _use(monkeypatch, _Context(mode))
    paths = [files[k] for k in (1, 2, 128)][:n]
    keywords = {} if mode == "turned" else {"tolerance": 31}
    got = PUBLIC[mode](paths, **keywords)
    assert len(got) == len(DOCUMENTED[mode]) + 1
    for mine, (shape, dtype) in zip(got, DOCUMENTED[mode] + [((), np.bool_)]):
        assert isinstance(mine, np.ndarray) and mine.shape == (n,) + shape and mine.dtype == dtype
    same = _views.view_signatures(mode, paths, 31, 0)
    assert all(np.array_equal(a, b) for a, b in zip(got, same))


@pytest.mark.parametrize("function", [trimmed.trimmed_signatures, turned_trimmed.turned_trimmed_signatures])
def test_the_tolerance_is_checked_before_anything_is_opened(monkeypatch, function):
    monkeypatch.setattr(_native, "get_context", lambda *a, **k: pytest.fail("a context was asked for"))
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="tolerance"):
            function(["x.png"], tolerance=bad)
