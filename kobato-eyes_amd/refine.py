"""SSIM refinement on the MI355X: drop-in for the reference's ``dup.refine``.

Mirrors src/dup/refine.py: ``refine_pair``, ``RefinementThresholds``, ``RefinedMatch``.  The
SSIM value comes from csrc/ke_ssim.hip (skimage's 7x7 uniform-window SSIM, float32).  ORB
(src/dup/refine.py:55-68) is outside this build's scope: ``orb_ratio`` is
always None and the decision is ``ssim >= thresholds.ssim`` alone.
"""
from __future__ import annotations

import importlib
import logging
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _native
from .formats import (AS_DECODED, LEAVE, NORMALISE, SHRINK, SHRINK_OVERSIZE, TURN_SHRINK, Offers, decoded_bytes_estimate,
                      oversize_enabled, seam_actions)
from .image_io import MAX_SIDE, load_rgb

_phash = importlib.import_module(".phash", __package__)   # the package also exports a function named phash

logger = logging.getLogger(__name__)


@dataclass(frozen=True)
class RefinementThresholds:
    ssim: float = 0.9
    orb: float = 0.15


@dataclass(frozen=True)
class RefinedMatch:
    file_id_a: int
    file_id_b: int
    ssim: Optional[float]
    orb_ratio: Optional[float]
    is_duplicate: bool
    reason: str


def _common_size(img_a, img_b) -> tuple[int, int]:
    """(min width, min height) of the two images (src/dup/refine.py:45-47)."""
    size = (min(img_a.width, img_b.width), min(img_a.height, img_b.height))
    if size[0] == 0 or size[1] == 0:
        size = (max(img_a.width, img_b.width), max(img_a.height, img_b.height))
    return size


def compute_ssim(img_a, img_b, *, device: int = 0) -> float:
    """SSIM of two PIL images of any two sizes (src/dup/refine.py:44-52).

    Both are brought to the common size the way the reference does -- ``ImageOps.fit(image.convert("L"), size,
    BICUBIC)``: centre crop to the aspect ratio, Pillow's fixed-point bicubic resize -- by ``ke_fit_luma_uniform``;
    the two luma planes stay in device memory for the SSIM kernel.
    """
    ctx = _native.get_context(device)
    w, h = _common_size(img_a, img_b)
    if w < 7 or h < 7:
        raise ValueError("win_size exceeds image extent")  # what skimage raises for tiny images
    planes = ctx.malloc(2 * w * h)
    try:
        for k, image in enumerate((img_a, img_b)):
            arr = _phash.image_to_array(image)
            channels = 1 if arr.ndim == 2 else arr.shape[2]
            ctx.fit_luma_uniform(arr, 1, arr.shape[1], arr.shape[0], channels, w, h, _native.FILTER_BICUBIC,
                                 out=planes + k * w * h)
        return float(ctx.ssim_pairs_uniform(planes, 2, w, h, 1, [0], [1])[0])
    finally:
        ctx.free(planes)


def ssim_pairs(images: np.ndarray, pair_a: Sequence[int], pair_b: Sequence[int], *, device: int = 0) -> np.ndarray:
    """Batched form: images (n,h,w[,c]) u8 of one size, SSIM for every (pair_a[k], pair_b[k])."""
    images = np.ascontiguousarray(images, dtype=np.uint8)
    n, h, w = images.shape[:3]
    ch = 1 if images.ndim == 3 else images.shape[3]
    return _native.get_context(device).ssim_pairs_uniform(images, n, w, h, ch, pair_a, pair_b)


def _decide(file_id_a: int, file_id_b: int, ssim_value: Optional[float], errors: list, cfg: RefinementThresholds) -> RefinedMatch:
    """The decision and ``reason`` text of src/dup/refine.py:100-117 (ORB left out)."""
    reasons: list[str] = []
    if ssim_value is not None and ssim_value >= cfg.ssim:
        reasons.append(f"ssim>={cfg.ssim}")
    reason = ", ".join(reasons or errors) if (reasons or errors) else "below thresholds"
    return RefinedMatch(file_id_a, file_id_b, ssim_value, None, bool(reasons), reason)


def _decode_on_gpu(ctx, need: list, placed: dict, buffers: list, count: dict, max_side: int = MAX_SIDE) -> None:
    """The files of ``need`` that a GPU decoder of formats.FORMATS takes and formats.seam_actions does not leave to the loader
    are decoded on the GPU and stay there, as the reference's loader would hand them over (src/utils/image_io.py:107-138):
    placed[path] = (device address, width, height), every buffer that holds one in ``buffers``.  Everything else is left
    for Pillow.

    With ``KE_GPU_REFINE_OVERSIZE=1`` files of any size stay: JPEG files are decoded at the scale the loader's ``draft`` picks
    (a 12 000 x 9 000 file is never held at full size), and what is still more than four times ``max_side`` is reduced by
    whole factors before the LANCZOS pass, as ``Image.thumbnail`` does (SHRINK_OVERSIZE)."""
    oversize = oversize_enabled()
    offers = Offers("refine", need, placed)
    for kind, paths in offers:
        if oversize and kind == "jpeg":
            dev, off, w, h, c, st, flags, denoms = ctx.decode_files_owned(paths, kind, draft_side=max_side)
        else:
            dev, off, w, h, c, st, flags = ctx.decode_files_owned(paths, kind)
            denoms = np.ones(len(paths), np.int32)
        offers.ran(kind, paths, st)
        if not dev:
            continue
        buffers.append(dev)
        action, orient = seam_actions(kind, "refine", w, h, c, st, flags, max_side, oversize=oversize)
        # the files the oversize route kept from the loader: shrunk from beyond the window, or drafted into it
        drafted = int(np.count_nonzero((denoms > 1) & (action != LEAVE) & (action != SHRINK_OVERSIZE)))
        if drafted:
            count["gpu_oversize"] = count.get("gpu_oversize", 0) + drafted
        ok = np.nonzero(action == AS_DECODED)[0]
        for k, o, ww, hh in zip(ok.tolist(), off[ok].tolist(), w[ok].tolist(), h[ok].tolist()):
            placed[paths[k]] = (dev + o, ww, hh)
        count["gpu_decodes"] += len(ok)
        # what the loader does to a file (src/utils/image_io.py:116-131) happens on the device as well: the EXIF orientation
        # applied (every camera writes one), RGBA composited over white
        fix = np.nonzero(action == NORMALISE)[0]
        if len(fix):
            dev2, off2, w2, h2 = ctx.normalise_rgb(dev, off[fix], w[fix], h[fix], c[fix], orient[fix])
            buffers.append(dev2)
            for k, o2, ww, hh in zip(fix.tolist(), off2.tolist(), w2.tolist(), h2.tolist()):
                placed[paths[k]] = (dev2 + int(o2), ww, hh)
            count["gpu_decodes"] += len(fix)
            count["gpu_normalised"] = count.get("gpu_normalised", 0) + len(fix)
        for k in np.nonzero((action == SHRINK) | (action == TURN_SHRINK) | (action == SHRINK_OVERSIZE))[0].tolist():
            addr, ww, hh, held = dev + int(off[k]), int(w[k]), int(h[k]), None
            try:
                if action[k] == TURN_SHRINK or (action[k] == SHRINK_OVERSIZE and orient[k] != 1):
                    held, o2, w2, h2 = ctx.normalise_rgb(dev, off[k:k + 1], w[k:k + 1], h[k:k + 1], c[k:k + 1], orient[k:k + 1])
                    addr, ww, hh = held + int(o2[0]), int(w2[0]), int(h2[0])
                if action[k] == SHRINK_OVERSIZE:
                    small, sw, sh, _ = ctx.thumbnail_rgb_reduced(addr, ww, hh, max_side)
                else:
                    small, sw, sh = ctx.thumbnail_rgb(addr, ww, hh, max_side)
            finally:
                if held is not None:
                    ctx.free(held)
            buffers.append(small)
            placed[paths[k]] = (small, sw, sh)
            count["gpu_decodes"] += 1
            key = "gpu_oversize" if action[k] == SHRINK_OVERSIZE else "gpu_shrunk"
            count[key] = count.get(key, 0) + 1


def _load(p: str, max_side: int = MAX_SIDE):
    img = load_rgb(p, max_side=max_side)
    if img is None:
        return None
    arr = _phash.image_to_array(img)
    return arr if arr.ndim == 3 and arr.shape[2] == 3 else None


def _upload(ctx, arrays: dict, placed: dict, buffers: list) -> None:
    """Images decoded by Pillow are uploaded next to the ones decoded on the GPU."""
    host = [(p, a) for p, a in arrays.items() if a is not None]
    if not host:
        return
    sizes = [(a.size + 15) & ~15 for _, a in host]
    flat = np.zeros(sum(sizes), np.uint8)
    at = 0
    dev = ctx.malloc(len(flat) + 64)
    buffers.append(dev)
    for (p, a), sz in zip(host, sizes):
        flat[at:at + a.size] = a.reshape(-1)
        placed[p] = (dev + at, a.shape[1], a.shape[0])
        at += sz
    ctx.memcpy(dev, flat, len(flat))


PLAIN, TURNED, TRIMMED, VIEWED = "plain", "turned", "trimmed", "viewed"
# what a mode of _refine_runs uses of a row's (trimmed_a, trimmed_b, orientation): (the flags, the orientation, its own counters)
_MODES = {PLAIN: (False, False, ()), TURNED: (False, True, ()), TRIMMED: (True, False, ("box_files", "crop_launches")),
          VIEWED: (True, True, ("box_files", "crop_launches", "turn_launches", "view_launches"))}


def _seam_boxes(ctx, pairs: Sequence[tuple], live: list, paths: list, index: dict, placed: dict, count: dict, tolerance: int):
    """The boxes of a trimmed run, (box_a, box_b) as int32[len(live), 4]: one ``ke_content_boxes`` call on the pictures that
    have a trimmed side, as they are placed on the device.  A side that is not trimmed, and a trimmed side whose picture has
    no box here, stays four zeros: the picture as it lies."""
    sides = [(n, 4 + s, index[str(pairs[k][2 + s])]) for n, k in enumerate(live) for s in (0, 1) if pairs[k][4 + s]]
    boxes = np.zeros((2, len(live), 4), np.int32)
    files = sorted({i for _, _, i in sides})
    if files:
        found, _ = ctx.content_boxes_on_device([placed[paths[i]][0] for i in files], [placed[paths[i]][1] for i in files],
                                               [placed[paths[i]][2] for i in files], 3, tolerance)
        row = {i: r for r, i in enumerate(files)}
        for n, item, i in sides:
            boxes[item - 4, n] = found[row[i]]
        count["box_files"] += len(files)
    return boxes[0], boxes[1]


def _score(ctx, pairs: Sequence[tuple], chunk: range, placed: dict, out: list, count: dict, cfg: RefinementThresholds,
           mode: str = PLAIN, tolerance: int = 48) -> None:
    """One library call for the pairs of this run (the library groups them: one fit launch per (source size, common size), one
    SSIM launch per common size).  A row is ``(id_a, id_b, path_a, path_b, trimmed_a, trimmed_b, orientation)``.  PLAIN:
    ``ke_ssim_pairs``.  The other modes: ``ke_ssim_pairs_viewed``, a's view against that orientation of b's view, with the
    content box, found here, of every flagged side where the mode has boxes, and the orientations where it has them."""
    live = []
    for k in chunk:
        pa, pb = pairs[k][2], pairs[k][3]
        if str(pa) not in placed or str(pb) not in placed:
            out[k] = None                                      # unreadable file: src/dup/refine.py:82-85
        else:
            live.append(k)
    if not live:
        return
    paths = list(placed)
    index = {p: i for i, p in enumerate(paths)}
    where = ([placed[p][0] for p in paths], [placed[p][1] for p in paths], [placed[p][2] for p in paths], 3,
             [index[str(pairs[k][2])] for k in live], [index[str(pairs[k][3])] for k in live])
    has_boxes, has_orientations, counters = _MODES[mode]
    box_a = box_b = None
    if has_boxes:
        box_a, box_b = _seam_boxes(ctx, pairs, live, paths, index, placed, count, tolerance)
    if mode == PLAIN:
        scores, status = ctx.ssim_pairs_on_device(*where)
    else:
        scores, status = ctx.ssim_pairs_viewed_on_device(*where, box_a, box_b, [int(pairs[k][6]) for k in live] if has_orientations else None)
    if not has_boxes:
        box_a = box_b = np.zeros((len(live), 4), np.int32)
    common, fits, made = set(), set(), {"crop_launches": False, "turn_launches": False, "view_launches": False}
    for n, (k, sc, st) in enumerate(zip(live, scores.tolist(), status.tolist())):
        fid_a, fid_b, pa, pb = pairs[k][:4]
        if st != 0:                                            # skimage raises for images smaller than its window
            logger.warning("SSIM refinement failed for %s and %s: win_size exceeds image extent", pa, pb)
            out[k] = _decide(fid_a, fid_b, None, ["ssim unavailable"], cfg)
            continue
        out[k] = _decide(fid_a, fid_b, float(sc), [], cfg)
        (_, wa, ha), (_, wb, hb) = placed[str(pa)], placed[str(pb)]
        o = int(pairs[k][6])
        # a box other than the whole picture (as it lies) is a source of its own, as a turned plane is
        cut_a, cut_b = (bool(b.any()) and tuple(b) != (0, 0, w, h) for b, w, h in ((box_a[n], wa, ha), (box_b[n], wb, hb)))
        if cut_a:
            wa, ha = int(box_a[n][2] - box_a[n][0]), int(box_a[n][3] - box_a[n][1])
        if cut_b:
            wb, hb = int(box_b[n][2] - box_b[n][0]), int(box_b[n][3] - box_b[n][1])
        if o & 4:                                              # crop, then turn
            wb, hb = hb, wb
        made["crop_launches"] |= cut_a or (cut_b and o == 0)
        made["turn_launches"] |= o != 0 and not cut_b
        made["view_launches"] |= o != 0 and cut_b
        size = (min(wa, wb), min(ha, hb))
        common.add(size)
        fits.update({((ha, wa), cut_a, size), ((hb, wb), o != 0 or cut_b, size)})
    count["fit_launches"] += len(fits)
    count["ssim_launches"] += len(common)
    for name in counters:
        if name in made:
            count[name] += int(made[name])


def refine_pairs(pairs: Sequence[tuple], *, thresholds: Optional[RefinementThresholds] = None, device: int = 0,
                 io_workers: int = 8, max_decoded_bytes: int = 1 << 30, stats: Optional[dict] = None,
                 devices: Optional[Sequence[int]] = None, max_side: int = MAX_SIDE, _after_run=None) -> list:
    """``refine_pair`` for a list of ``(file_id_a, file_id_b, path_a, path_b)``: the same ``RefinedMatch`` (or ``None``)
    per pair, in input order -- but every file is decoded once however many pairs share it, and the kernels see groups
    instead of single pairs: one ``ke_fit_luma_uniform`` launch per (source size, channels, common size) and one
    ``ke_ssim_pairs_uniform`` launch per common size.  The reference's loop decodes both files of every pair again and
    runs the metric pair by pair (src/dup/refine.py:82-98).

    Pairs are worked off in runs whose decoded files stay below ``max_decoded_bytes``.  ``stats`` (optional dict)
    receives the launch and decode counts.  ``max_side``: the side the loader shrinks a larger picture to
    (``safe_load_image(max_side=...)``), for Pillow's route and the GPU's alike; with ``KE_GPU_REFINE_OVERSIZE=1`` the files
    that are shrunk on the device from beyond the window of ``formats.seam_actions``, and the JPEG files drafted into or below
    it, are counted as ``gpu_oversize`` (``formats.OVERSIZE_*``: the bounds beyond which a file still takes the loader).

    ``devices`` (e.g. ``[0, 1, 2]``; at most 15 entries): the pairs are cut into one contiguous block of about equal
    ``decoded_bytes_estimate`` per entry, and one worker process per entry runs this function on its block on its own device
    with ``io_workers // N`` loaders (``ranks.py``).  The answers are those of ``devices=None`` -- the SSIM partial sums are
    integers --, in input order; ``stats`` holds the workers' counters summed, so ``decodes`` counts a file once per worker
    that needed it.  A worker that dies or falls silent ends the call with ``RuntimeError``.
    """
    if devices is not None:
        from . import ranks

        return ranks.refine_pairs(pairs, devices, thresholds=thresholds, io_workers=io_workers,
                                  max_decoded_bytes=max_decoded_bytes, stats=stats, max_side=max_side)
    rows = [(*p[:4], False, False, 0) for p in pairs]
    return _refine_runs(rows, PLAIN, thresholds, device, io_workers, max_decoded_bytes, stats, max_side, _after_run)


def _refine_runs(pairs: Sequence[tuple], mode: str, thresholds, device: int, io_workers: int, max_decoded_bytes: int,
                 stats: Optional[dict], max_side: int, _after_run=None, tolerance: int = 48) -> list:
    """The run loop of refine_pairs, refine_turned_pairs, refine_trimmed_pairs and refine_turned_trimmed_pairs (``mode``: PLAIN,
    TURNED, TRIMMED, VIEWED; rows ``(id_a, id_b, path_a, path_b, trimmed_a, trimmed_b, orientation)`` whatever the mode): decode
    what a run of pairs needs, once per file and within the budget, score the run with one library call, free, go on."""
    from concurrent.futures import ThreadPoolExecutor

    cfg = thresholds or RefinementThresholds()
    ctx = _native.get_context(device)
    out: list = [None] * len(pairs)
    count = {"decodes": 0, "gpu_decodes": 0, "fit_launches": 0, "ssim_launches": 0, "pairs": len(pairs)}
    count.update(dict.fromkeys(_MODES[mode][2], 0))
    with ThreadPoolExecutor(max_workers=max(1, io_workers)) as pool:
        start = 0
        while start < len(pairs):
            need, size_est, stop = [], 0, start                    # grow the run until the decode budget is reached
            seen: set = set()
            while stop < len(pairs) and (size_est < max_decoded_bytes or stop == start):
                for p in (str(pairs[stop][2]), str(pairs[stop][3])):
                    if p not in seen:
                        seen.add(p)
                        need.append(p)
                        size_est += decoded_bytes_estimate(p)
                stop += 1
            placed: dict = {}
            buffers: list = []
            try:
                _decode_on_gpu(ctx, need, placed, buffers, count, max_side)
                rest = [p for p in need if p not in placed]
                arrays = dict(zip(rest, pool.map(lambda p: _load(p, max_side), rest)))
                count["decodes"] += len(need)
                _upload(ctx, arrays, placed, buffers)
                _score(ctx, pairs, range(start, stop), placed, out, count, cfg, mode, tolerance)
            finally:
                for dev in buffers:
                    ctx.free(dev)
            start = stop
            if _after_run is not None:                             # a rank worker says how far it has come
                _after_run(stop)
    if stats is not None:
        stats.update(count)
    return out


def refine_turned_pairs(pairs: Sequence[tuple], *, thresholds: Optional[RefinementThresholds] = None, device: int = 0,
                        io_workers: int = 8, max_decoded_bytes: int = 1 << 30, stats: Optional[dict] = None,
                        max_side: int = MAX_SIDE) -> list:
    """``refine_pairs`` for a list of ``(file_id_a, file_id_b, path_a, path_b, orientation)``: file a is scored against
    orientation ``orientation`` (0..7, ``turned.ORIENTATIONS``) of file b, as ``refine_pairs`` would score a against a file
    that holds b turned that way.  A capability of this library only: the reference has no turned duplicates.

    Both files are decoded as they lie (the same decode runs, budget and loader fallback as ``refine_pairs``, the same
    ``stats``); b is turned on the device, luma only, once per distinct (file, orientation) of a run (``ke_turn_luma`` inside
    ``ke_ssim_pairs_turned``).  Luma commutes with the turn and the resampler is bit-exact with Pillow on every source, so the
    score is the one the turned file would get, bit for bit.  Returns a ``RefinedMatch`` or ``None`` (unreadable file) per
    pair, in input order.

    There is no ``devices=``: ``ranks.refine_pairs`` ships 4-tuples to its workers.  An orientation outside 0..7 is a
    ``ValueError`` before anything is decoded."""
    for pair in pairs:
        if not 0 <= int(pair[4]) < 8:
            raise ValueError(f"orientation {pair[4]} outside 0..7")
    rows = [(*p[:4], False, False, int(p[4])) for p in pairs]
    return _refine_runs(rows, TURNED, thresholds, device, io_workers, max_decoded_bytes, stats, max_side)


def refine_trimmed_pairs(pairs: Sequence[tuple], *, tolerance: int = 48, thresholds: Optional[RefinementThresholds] = None, device: int = 0,
                         io_workers: int = 8, max_decoded_bytes: int = 1 << 30, stats: Optional[dict] = None,
                         max_side: int = MAX_SIDE) -> list:
    """``refine_pairs`` for a list of ``(file_id_a, file_id_b, path_a, path_b, trimmed_a, trimmed_b)``: a side whose flag is
    set takes part with its content box (include/keyes.h, ``ke_content_boxes`` at ``tolerance``) instead of the whole picture,
    as ``refine_pairs`` would score a file that holds Pillow's ``crop`` of it.  A capability of this library only: the
    reference has no bordered copies.

    Both files are decoded as they lie (the same decode runs, budget and loader fallback as ``refine_pairs``, the same
    ``stats``).  The boxes are made here, per run, by one ``ke_content_boxes`` call on the pictures as they are placed on the
    device, not taken from ``trimmed.trimmed_signatures``: this seam's loader applies the EXIF orientation, composites RGBA
    over white and shrinks oversized files, so a box found at the hashing seam may describe another pixel grid.  A flagged
    side whose picture has no box here is scored as it lies.  Then one ``ke_ssim_pairs_boxed`` call: every distinct (file,
    box) is cut out once, luma only (``ke_crop_luma``), and the crop is fitted -- crop first, then fit, so that the margin
    cannot bleed into the crop's edge through the resampler's taps.  Luma is per pixel and the resampler is bit-exact with
    Pillow on every source, so the score is the one the cropped file would get, bit for bit.  ``stats`` also receives
    ``box_files`` (pictures whose box was looked for) and ``crop_launches``.  Returns a ``RefinedMatch`` or ``None``
    (unreadable file) per pair, in input order.

    There is no ``devices=``: ``ranks.refine_pairs`` ships 4-tuples to its workers.  A tolerance outside 0..255 is a
    ``ValueError`` before anything is decoded."""
    if not 0 <= int(tolerance) <= 255:
        raise ValueError(f"tolerance {tolerance} outside 0..255")
    rows = [(*p[:6], 0) for p in pairs]
    return _refine_runs(rows, TRIMMED, thresholds, device, io_workers, max_decoded_bytes, stats, max_side, tolerance=int(tolerance))


def refine_turned_trimmed_pairs(pairs: Sequence[tuple], *, tolerance: int = 48, thresholds: Optional[RefinementThresholds] = None,
                                device: int = 0, io_workers: int = 8, max_decoded_bytes: int = 1 << 30, stats: Optional[dict] = None,
                                max_side: int = MAX_SIDE) -> list:
    """``refine_pairs`` for a list of ``(file_id_a, file_id_b, path_a, path_b, trimmed_a, trimmed_b, orientation)``: a's view is
    scored against orientation ``orientation`` (0..7, ``turned.ORIENTATIONS``) of b's view, a view being the file's content box
    (include/keyes.h, ``ke_content_boxes`` at ``tolerance``) where its flag is set and the whole picture otherwise -- crop, then
    turn, then fit -- as ``refine_pairs`` would score files that hold Pillow's ``crop(box)`` of a and ``crop(box).transpose(...)``
    of b.  A capability of this library only: the reference has neither bordered nor turned copies.

    Both files are decoded as they lie (the same decode runs, budget and loader fallback as ``refine_pairs``, the same
    ``stats``).  The boxes are made here, per run, on the pictures as they are placed on the device, as
    ``refine_trimmed_pairs`` makes them and for its reason; a flagged side whose picture has no box here is scored as it lies.
    Then one ``ke_ssim_pairs_viewed`` call per run: every distinct (file, box, orientation) is made once, luma only, by one launch
    per kind of view -- a box as it lies (``ke_crop_luma``), a whole picture turned (``ke_turn_luma``), a box turned
    (``ke_crop_turn_luma``).  Luma is per pixel, the turn a permutation and the resampler bit-exact with Pillow on every source,
    so the planes the score is taken from are those of the cropped and turned files, byte for byte.  ``stats`` also receives
    ``box_files`` (pictures whose box was looked for), ``crop_launches``, ``turn_launches`` and ``view_launches`` (the three
    kernels above, in that order).  Returns a ``RefinedMatch`` or ``None`` (unreadable file) per pair, in input order.

    There is no ``devices=``: ``ranks.refine_pairs`` ships 4-tuples to its workers.  A tolerance outside 0..255 or an
    orientation outside 0..7 is a ``ValueError`` before anything is decoded."""
    if not 0 <= int(tolerance) <= 255:
        raise ValueError(f"tolerance {tolerance} outside 0..255")
    for pair in pairs:
        if not 0 <= int(pair[6]) < 8:
            raise ValueError(f"orientation {pair[6]} outside 0..7")
    return _refine_runs(pairs, VIEWED, thresholds, device, io_workers, max_decoded_bytes, stats, max_side, tolerance=int(tolerance))


def refine_pair(file_id_a: int, file_id_b: int, path_a, path_b, *, thresholds: Optional[RefinementThresholds] = None,
                device: int = 0) -> Optional[RefinedMatch]:
    image_a, image_b = load_rgb(path_a), load_rgb(path_b)
    if image_a is None or image_b is None:
        return None
    cfg = thresholds or RefinementThresholds()
    ssim_value: Optional[float] = None
    errors: list[str] = []
    try:
        ssim_value = compute_ssim(image_a, image_b, device=device)
    except Exception as exc:
        logger.warning("SSIM refinement failed for %s and %s: %s", path_a, path_b, exc)
        errors.append("ssim unavailable")
    return _decide(file_id_a, file_id_b, ssim_value, errors, cfg)


__all__ = ["RefinementThresholds", "RefinedMatch", "refine_pair", "refine_pairs", "refine_turned_pairs", "refine_trimmed_pairs", "refine_turned_trimmed_pairs",
           "compute_ssim",
           "ssim_pairs"]
