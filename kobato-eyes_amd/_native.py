"""ctypes binding of libkeyes_hip.so (include/keyes.h).

The product path has NO CPU fallback: if the shared library is missing, or no gfx950 device
is visible, every entry point raises ``RuntimeError`` -- the same way the reference's
``phash`` raises when OpenCV is missing (src/sig/phash.py:35-36).
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional, Sequence

import numpy as np

from .formats import FORMATS, KINDS

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KE_LIBKEYES") or os.path.join(_PKG_DIR, "libkeyes_hip.so")   # KE_LIBKEYES: a build variant (benchmarks)

KE_OK = 0
EDGE_DTYPE = np.dtype([("a", "<i8"), ("b", "<i8"), ("h", "<i4"), ("bands", "<i4")])

# The hash calls that stand behind a decode, by mode: (C function, whether it takes ``tolerance``, its outputs as (name, trailing
# shape, dtype)).  Each is f(ctx, pixels, offsets, widths, heights, channels, n, [tolerance,] *outputs, status); ``has`` comes
# back as bytes and is handed on as bool.  A further view of a picture is a row here (Context._hash_views_at).
HASH_CALLS = {
    "plain": ("ke_hash_images", False, (("phash", (), np.uint64), ("dhash", (), np.uint64))),
    "turned": ("ke_hash_images_turned", False, (("turned", (8,), np.uint64),)),
    "trimmed": ("ke_hash_images_trimmed", True, (("phash", (), np.uint64), ("boxes", (4,), np.int32), ("has", (), np.uint8))),
    "turned_trimmed": ("ke_hash_images_turned_trimmed", True, (("turned", (8,), np.uint64), ("trimmed_turned", (8,), np.uint64),
                                                               ("boxes", (4,), np.int32), ("has", (), np.uint8))),
}


def hash_outputs(mode: str, n: int, leave: Sequence[str] = ()) -> dict:
    """{name: zeros[n, ...]} for the outputs of HASH_CALLS[mode] as a caller sees them (``has`` bool; None for a name in
    ``leave``), then "status": int32[n]."""
    out = {name: None if name in leave else np.zeros((n,) + shape, bool if name == "has" else dtype)
           for name, shape, dtype in HASH_CALLS[mode][2]}
    out["status"] = np.zeros(n, np.int32)
    return out

# every symbol include/keyes.h declares (tests check the library exports all of them)
FILTER_LANCZOS, FILTER_BILINEAR, FILTER_BICUBIC = 0, 1, 2   # include/keyes.h KE_FILTER_*

EXPORTS = (
    "ke_abi_version", "ke_create", "ke_create_error", "ke_destroy", "ke_last_error", "ke_set_stream",
    "ke_get_stream", "ke_synchronize", "ke_device_info", "ke_malloc", "ke_free", "ke_memcpy",
    "ke_hash_images", "ke_hash_uniform", "ke_hash_images_ex", "ke_hash_uniform_ex", "ke_luma_tiles_uniform", "ke_hamming_scan",
    "ke_hamming_scan_from", "ke_hamming_scan_cross", "ke_hamming_scan_exact", "ke_hamming_nearest", "ke_tiles_turned", "ke_hash_images_turned", "ke_band_pairs_after_size",
    "ke_content_boxes", "ke_crop_pack", "ke_hash_images_trimmed", "ke_crop_luma", "ke_ssim_pairs_boxed",
    "ke_crop_turn_luma", "ke_ssim_pairs_viewed", "ke_hash_images_turned_trimmed",
    "ke_stage_create", "ke_stage_create_shared", "ke_stage_destroy", "ke_stage_acquire", "ke_stage_submit_hash", "ke_stage_wait",
    "ke_comm_unique_id", "ke_comm_create", "ke_comm_destroy", "ke_allgather_u64", "ke_allgather_hashes", "ke_allgather_edges",
    "ke_interleave_shards", "ke_host_alloc", "ke_host_free", "ke_host_pack", "ke_host_read_files",
    "ke_normalise_rgb", "ke_thumbnail_rgb", "ke_thumbnail_rgb_box", "ke_reduce_rgb", "ke_jpeg_decode_scaled", "ke_jpeg_last_split", "ke_cluster_labels", "ke_ssim_pairs_uniform", "ke_ssim_pairs", "ke_ssim_pairs_turned", "ke_turn_luma", "ke_ssim_set_mode",
    "ke_resize_luma_uniform", "ke_fit_luma_uniform", "ke_tile_ahash", "ke_sad_pairs", "ke_synth_rgb", "ke_synth_rgb_indexed",
    "ke_synth_hashes", "ke_last_kernel_ms", "ke_last_decode_sub_batches", "ke_last_scan_path", "ke_last_resize_plan", "ke_last_ssim_plan",
) + tuple(f"ke_{kind}_{call}" for kind in KINDS for call in ("probe", "decode", "caveats"))

_lib: Optional[C.CDLL] = None
_lib_lock = threading.Lock()


class _BatchTooLarge(Exception):
    """A decode batch whose compressed or decoded bytes exceed the context's limits: the caller halves it."""


class NativeUnavailable(RuntimeError):
    """libkeyes_hip.so (or a gfx950 device) is not available."""


def _share_the_hip_runtime_with_torch() -> None:
    """PyTorch's ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 / librccl.  One process must run on ONE HIP
    runtime: if this library bound /opt/rocm's copy and PyTorch (or its RCCL) were loaded afterwards, the second copy would
    see no initialised device.  So when PyTorch is installed its runtime is mapped first (without importing torch); the
    loader then resolves libkeyes_hip.so's dependency to it by soname.  KE_SYSTEM_ROCM=1 keeps the system copy."""
    import importlib.util
    import sys

    if "torch" in sys.modules or os.environ.get("KE_SYSTEM_ROCM"):
        return                      # torch already brought its runtime (same effect) / the caller wants /opt/rocm's
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library() -> C.CDLL:
    """Load libkeyes_hip.so and declare the prototypes.  Does not touch the GPU."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        _share_the_hip_runtime_with_torch()
        if not os.path.exists(LIB_PATH):
            raise NativeUnavailable(
                f"{LIB_PATH} is missing: build it with kobato-eyes_amd/build.sh (hipcc, gfx950). "
                "There is no CPU fallback for the hash/scan path."
            )
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as exc:  # e.g. libamdhip64 not found
            raise NativeUnavailable(f"cannot load {LIB_PATH}: {exc}") from exc
        vp, i32, i64, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
        for name in EXPORTS:                                 # all but the few below return a KE_* code
            getattr(lib, name).restype = C.c_int
        lib.ke_create.argtypes = [C.c_int]
        lib.ke_create.restype = vp
        lib.ke_create_error.restype = C.c_char_p
        lib.ke_destroy.argtypes = [vp]
        lib.ke_destroy.restype = None
        lib.ke_last_error.argtypes = [vp]
        lib.ke_last_error.restype = C.c_char_p
        lib.ke_set_stream.argtypes = [vp, vp]
        lib.ke_get_stream.argtypes = [vp]
        lib.ke_get_stream.restype = vp
        lib.ke_synchronize.argtypes = [vp]
        lib.ke_device_info.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(i32), C.POINTER(i64)]
        lib.ke_malloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        lib.ke_free.argtypes = [vp, vp]
        lib.ke_memcpy.argtypes = [vp, vp, vp, C.c_size_t]
        lib.ke_hash_images.argtypes = [vp, vp, vp, vp, vp, i32, i64, vp, vp, vp]
        lib.ke_hash_uniform.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp]
        lib.ke_hash_images_ex.argtypes = [vp, vp, vp, vp, vp, i32, i64, vp, vp, vp, vp]
        lib.ke_hash_uniform_ex.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp, vp]
        lib.ke_luma_tiles_uniform.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp]
        lib.ke_stage_create.argtypes = [vp, C.c_size_t, i64, i32]
        lib.ke_stage_create_shared.argtypes = [vp, vp, C.c_size_t, i64, i32]
        lib.ke_stage_destroy.argtypes = [vp]
        lib.ke_stage_acquire.argtypes = [vp, C.POINTER(i32), C.POINTER(vp), C.POINTER(C.c_size_t)]
        lib.ke_stage_submit_hash.argtypes = [vp, i32, vp, vp, vp, vp, i64, vp, vp, vp, vp]
        lib.ke_stage_wait.argtypes = [vp, i32]
        lib.ke_comm_unique_id.argtypes = [vp]
        lib.ke_comm_create.argtypes = [vp, vp, i32, i32, C.POINTER(vp)]
        lib.ke_comm_destroy.argtypes = [vp, vp]
        lib.ke_allgather_u64.argtypes = [vp, vp, i32, vp, i64, vp]
        lib.ke_allgather_hashes.argtypes = [vp, vp, i32, vp, i64, vp]
        lib.ke_allgather_edges.argtypes = [vp, vp, i32, vp, i64, vp, i64, C.POINTER(i64), vp]
        lib.ke_interleave_shards.argtypes = [vp, vp, i32, i64, vp]
        lib.ke_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
        lib.ke_host_free.argtypes = [vp, vp]
        lib.ke_host_pack.argtypes = [vp, vp, vp, vp, i64]
        lib.ke_host_read_files.argtypes = [vp, i64, vp, C.c_uint64, vp, vp, C.POINTER(C.c_uint64)]
        for kind in KINDS:
            getattr(lib, f"ke_{kind}_probe").argtypes = [vp, vp, vp, i64, vp, vp, vp, vp]
            getattr(lib, f"ke_{kind}_decode").argtypes = [vp, vp, vp, vp, i64, vp, vp, vp]
            getattr(lib, f"ke_{kind}_caveats").argtypes = [vp, vp, vp, i64, vp]
        lib.ke_normalise_rgb.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, vp]
        lib.ke_thumbnail_rgb.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp]
        lib.ke_thumbnail_rgb_box.argtypes = [vp, vp, i32, i32, i32, i32, i32, vp, vp]
        lib.ke_reduce_rgb.argtypes = [vp, vp, i32, i32, i32, i32, vp]
        lib.ke_jpeg_decode_scaled.argtypes = [vp, vp, vp, vp, i64, vp, vp, vp, vp]
        lib.ke_jpeg_last_split.argtypes = [vp, vp, vp]
        lib.ke_band_pairs_after_size.argtypes = [vp, vp, vp, i64, i32, i32, dbl, i64, vp]
        lib.ke_hamming_scan.argtypes = [vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, dbl, i64, vp, i64,
                                        C.POINTER(i64), vp]
        lib.ke_hamming_scan_from.argtypes = [vp, vp, vp, vp, i64, i64, i32, i32, i32, i32, i32, dbl, i64, vp, i64,
                                             C.POINTER(i64), vp]
        lib.ke_hamming_scan_cross.argtypes = lib.ke_hamming_scan_from.argtypes
        lib.ke_hamming_scan_exact.argtypes = [vp, vp, vp, vp, i64, i64, i32, i32, i32, i32, i32, i32, dbl, vp, i64, vp, vp]
        lib.ke_hamming_nearest.argtypes = [vp, vp, vp, i64, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp]
        lib.ke_tiles_turned.argtypes = [vp, vp, i64, vp]
        lib.ke_hash_images_turned.argtypes = [vp, vp, vp, vp, vp, i32, i64, vp, vp]
        lib.ke_content_boxes.argtypes = [vp, vp, vp, vp, vp, i32, i64, i32, vp, vp]
        lib.ke_crop_pack.argtypes = [vp, vp, vp, vp, vp, i32, vp, i64, vp, vp]
        lib.ke_hash_images_trimmed.argtypes = [vp, vp, vp, vp, vp, i32, i64, i32, vp, vp, vp, vp]
        lib.ke_crop_luma.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, vp]
        lib.ke_ssim_pairs_boxed.argtypes = [vp, vp, vp, vp, vp, i32, i64, vp, vp, vp, vp, i64, vp, vp]
        lib.ke_crop_turn_luma.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp]
        lib.ke_ssim_pairs_viewed.argtypes = [vp, vp, vp, vp, vp, i32, i64, vp, vp, vp, vp, vp, i64, vp, vp]
        lib.ke_hash_images_turned_trimmed.argtypes = [vp, vp, vp, vp, vp, i32, i64, i32, vp, vp, vp, vp, vp]
        lib.ke_cluster_labels.argtypes = [vp, i64, i64, vp]
        lib.ke_ssim_pairs_uniform.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp, i64, vp]
        lib.ke_ssim_set_mode.argtypes = [vp, i32]
        lib.ke_ssim_pairs.argtypes = [vp, vp, vp, vp, vp, i32, i64, vp, vp, i64, vp, vp]
        lib.ke_ssim_pairs_turned.argtypes = [vp, vp, vp, vp, vp, i32, i64, vp, vp, vp, i64, vp, vp]
        lib.ke_turn_luma.argtypes = [vp, vp, vp, vp, vp, vp, vp, i64, vp, vp]
        lib.ke_resize_luma_uniform.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, i32, vp]
        lib.ke_fit_luma_uniform.argtypes = [vp, vp, i64, i32, i32, i32, i32, i32, i32, vp]
        lib.ke_tile_ahash.argtypes = [vp, vp, i64, i32, i32, vp]
        lib.ke_sad_pairs.argtypes = [vp, vp, i64, i64, vp, vp, i64, vp]
        lib.ke_synth_rgb.argtypes = [vp, u64, i64, i64, i32, i32, vp]
        lib.ke_synth_rgb_indexed.argtypes = [vp, u64, vp, i64, i32, i32, vp]
        lib.ke_synth_hashes.argtypes = [vp, u64, i64, vp]
        lib.ke_last_kernel_ms.argtypes = [vp, i32]
        lib.ke_last_kernel_ms.restype = dbl
        lib.ke_last_decode_sub_batches.argtypes = [vp]
        lib.ke_last_decode_sub_batches.restype = C.c_int64
        lib.ke_last_scan_path.argtypes = [vp]
        lib.ke_last_scan_path.restype = i32
        lib.ke_last_resize_plan.argtypes = [vp, vp]
        lib.ke_last_ssim_plan.argtypes = [vp, vp]
        _lib = lib
        return lib


def _addr(buf) -> Optional[int]:
    """Address of a host ndarray, a raw device pointer (int) or None."""
    if buf is None:
        return None
    if isinstance(buf, np.ndarray):
        return buf.ctypes.data
    if isinstance(buf, int):
        return buf
    if hasattr(buf, "data_ptr"):  # torch tensor (host or device): plumbing only
        return int(buf.data_ptr())
    raise TypeError(f"unsupported buffer type {type(buf)!r}")


def _leave_bombs_to_pillow(w, h, st, sizes) -> None:
    """Every decode here stands in for an ``Image.open``, which raises DecompressionBombError on an image of more than twice
    ``Image.MAX_IMAGE_PIXELS`` pixels: such files are marked unsupported (1) and hidden from the decoder (size 0: it reports
    them as not decodable and writes nothing), so that the caller's Pillow route raises as the reference's does.  The live
    value counts (safe_load_image changes it while it runs); None = no cap."""
    try:
        from PIL import Image
    except ModuleNotFoundError:  # pragma: no cover
        return
    cap = Image.MAX_IMAGE_PIXELS
    if cap is not None:
        bombs = (st == 0) & (w.astype(np.int64) * h > 2 * int(cap))
        st[bombs] = 1
        sizes[bombs] = 0


def draft_scale(widths, heights, max_side: int):
    """The denominators ``im.draft("RGB", (max_side, max_side))`` sets libjpeg up with, per file (int32): the largest of 8, 4,
    2, 1 that is at most min(width // max_side, height // max_side) -- 1 below twice ``max_side`` on either side (PIL
    JpegImagePlugin.draft; the reference's loader, src/utils/image_io.py:86-88)."""
    q = np.minimum(np.asarray(widths, np.int64) // max_side, np.asarray(heights, np.int64) // max_side)
    return np.select([q >= 8, q >= 4, q >= 2], [8, 4, 2], 1).astype(np.int32)


def thumbnail_size(width: int, height: int, box: int):
    """The size ``Image.thumbnail((box, box))`` gives a width x height image (aspect preserved; PIL/Image.py
    ``preserve_aspect_ratio``)."""
    import math

    def round_aspect(number, key):
        return max(min(math.floor(number), math.ceil(number), key=key), 1)

    x = y = box
    aspect = width / height
    if x / y >= aspect:
        x = round_aspect(y * aspect, key=lambda n: abs(aspect - n / y))
    else:
        y = round_aspect(x / aspect, key=lambda n: 0 if n == 0 else abs(aspect - x / n))
    return x, y


NOT_LAID = np.uint64(0xFFFFFFFFFFFFFFFF)       # lay_out's offset of an item that has no place in the buffer


def lay_out(nbytes, keys=None, absent=None):
    """Byte offsets of items of ``nbytes`` (int64 array) in one buffer, and the bytes they take together (see keyes.h).
    Without ``keys`` the items lie in input order, each on a 16-byte boundary.  With ``keys`` (arrays as np.lexsort takes them:
    the last one sorts first) they lie in that order, items of equal keys back to back without padding -- each such group can
    go to the uniform-batch kernels as it is -- and a group starts on 16 bytes.  ``absent``: a mask of items that sort behind
    all others; they and every item of no bytes get NOT_LAID."""
    n = len(nbytes)
    offsets = np.zeros(n, np.uint64)
    if keys is None:
        padded = (nbytes + 15) & ~np.int64(15)
        offsets[1:] = np.cumsum(padded[:-1]).astype(np.uint64)
        return offsets, int(padded.sum())
    if n == 0:
        return offsets, 0
    order = np.lexsort(tuple(keys) if absent is None else tuple(keys) + (absent,))
    size = nbytes[order].astype(np.int64)
    cols = np.stack([np.asarray(k)[order] for k in keys], 1)
    first = np.ones(n, bool)                                         # the items that begin a group
    first[1:] = (cols[1:] != cols[:-1]).any(1)
    group = np.cumsum(first) - 1
    before = np.cumsum(size) - size                                  # bytes of the items laid before this one, unpadded
    taken = np.add.reduceat(size, np.nonzero(first)[0])              # a group's bytes; its start: the padded groups before it
    padded = (taken + 15) & ~np.int64(15)
    start = np.cumsum(padded) - padded
    offsets[order] = (start[group] + before - before[first][group]).astype(np.uint64)
    if absent is not None:
        offsets[nbytes == 0] = NOT_LAID
    return offsets, int(start[-1] + taken[-1])


def runs_laid_out(offsets, keys):
    """lay_out's groups back from its offsets: index arrays of the items laid out, one per run of equal ``keys``, in buffer order."""
    laid = np.nonzero(offsets != NOT_LAID)[0]
    laid = laid[np.argsort(offsets[laid], kind="stable")]
    cols = np.stack([np.asarray(k)[laid] for k in keys], 1)
    return np.split(laid, np.nonzero((cols[1:] != cols[:-1]).any(1))[0] + 1)


def _pack_images(images):
    """Host images of one channel count in one array, each on a 16-byte boundary: (flat, offsets, widths, heights, channels)."""
    chans = {1 if im.ndim == 2 else im.shape[2] for im in images}
    if len(chans) != 1:
        raise ValueError("all images of one call must share the channel count")
    ch = chans.pop()
    widths = np.array([im.shape[1] for im in images], np.int32)
    heights = np.array([im.shape[0] for im in images], np.int32)
    sizes = widths.astype(np.int64) * heights * ch
    offsets, total = lay_out(sizes)
    flat = np.zeros(total, np.uint8)
    for im, off, sz in zip(images, offsets, sizes):
        flat[int(off):int(off) + int(sz)] = np.ascontiguousarray(im, dtype=np.uint8).reshape(-1)
    return flat, offsets, widths, heights, ch


def _base_and_offsets(pointers):
    """Device images, each at its own address, as one buffer: (the lowest address, every image's uint64 offset from it)."""
    ptrs = np.asarray(pointers, np.uint64)
    base = int(ptrs.min())
    return base, np.ascontiguousarray(ptrs - np.uint64(base))


class _Files:
    """Files packed in host memory, as the probe and decode calls take them: file i is ``flat[offsets[i]:offsets[i] + sizes[i]]``
    (size 0 = unreadable).  ``probed``: (kind, lo, hi) -> (widths, heights, channels, status) where the headers of files lo..hi
    of the batch this one was cut from (``part``) have been parsed already.  Made from bytes (Context._packed), from paths
    (Context._read_files_into) or as a part of a batch read ahead (FilesAhead)."""

    def __init__(self, flat, offsets, sizes, probed=None, first: int = 0) -> None:
        self.flat, self.offsets, self.sizes, self._first = flat, offsets, sizes, first
        self.probed = {} if probed is None else probed

    def __len__(self) -> int:
        return len(self.sizes)

    def part(self, lo: int, hi: int) -> "_Files":
        """Files lo..hi, with sizes of their own (a decode call hides files by their size)."""
        return _Files(self.flat, np.ascontiguousarray(self.offsets[lo:hi]), np.array(self.sizes[lo:hi], np.uint64), self.probed, self._first + lo)


class FilesAhead(_Files):
    """The files of a batch in one of a context's read-ahead buffers (Context.read_files_ahead).  ``release()`` hands the
    buffer back."""

    def __init__(self, ctx, slot: int, files: _Files) -> None:
        super().__init__(files.flat, files.offsets, files.sizes)
        self._ctx, self._slot = ctx, slot

    def release(self) -> None:
        if self._ctx is not None:
            self._ctx._ahead[self._slot][2] = False
            self._ctx, self.flat = None, None


def _in_halves(run, lo: int, hi: int) -> list:
    """[run(lo, hi)], or the same for the two halves of lo..hi -- and theirs -- where a call is _BatchTooLarge."""
    try:
        return [run(lo, hi)]
    except _BatchTooLarge:
        mid = lo + (hi - lo) // 2
        return _in_halves(run, lo, mid) + _in_halves(run, mid, hi)


class Context:
    """One ke_ctx: a device, a stream, scratch buffers.  Not re-entrant."""

    def __init__(self, device: int = 0) -> None:
        self._lib = load_library()
        self._h = self._lib.ke_create(int(device))
        if not self._h:
            msg = self._lib.ke_create_error().decode("utf-8", "replace")
            raise NativeUnavailable(f"ke_create({device}) failed: {msg}")
        self.device = int(device)
        self._lock = threading.RLock()
        self._pack = [0, 0]                                  # the packing buffer: [page-locked ptr, capacity]
        self._decoded_ptr, self._decoded_cap = 0, 0
        self._ahead = [[0, 0, False], [0, 0, False]]         # read-ahead buffers: [page-locked ptr, capacity, taken]
        self._ahead_lock = threading.Lock()
        self.decode_kernel_ms = 0.0        # kernel time of every ke_jpeg_decode / ke_png_decode call so far (a batch beyond the limits is several)
        # a decode call beyond these is split in halves: compressed bytes in page-locked memory, decoded pixels on the device
        self.pack_limit = int(os.environ.get("KE_PACK_LIMIT_BYTES", str(16 << 30)))
        self.decode_limit = int(os.environ.get("KE_DECODE_LIMIT_BYTES", str(48 << 30)))

    # -- lifetime ---------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_h", None):
            if getattr(self, "_decoded_ptr", 0):
                self._lib.ke_free(self._h, self._decoded_ptr)
                self._decoded_ptr, self._decoded_cap = 0, 0
            for buf in [getattr(self, "_pack", [0, 0])] + getattr(self, "_ahead", []):
                if buf[0]:
                    self._lib.ke_host_free(self._h, buf[0])
                    buf[0], buf[1] = 0, 0
            self._lib.ke_destroy(self._h)
            self._h = None

    def __del__(self) -> None:  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str) -> None:
        if rc != KE_OK:
            msg = self._lib.ke_last_error(self._h).decode("utf-8", "replace")
            if rc == -1:
                raise ValueError(f"{what}: {msg}")
            raise RuntimeError(f"{what} failed (rc={rc}): {msg}")

    # -- plumbing ---------------------------------------------------------------------------
    def set_stream(self, hip_stream: Optional[int]) -> None:
        self._check(self._lib.ke_set_stream(self._h, hip_stream), "ke_set_stream")

    def synchronize(self) -> None:
        self._check(self._lib.ke_synchronize(self._h), "ke_synchronize")

    def device_info(self) -> dict:
        name = C.create_string_buffer(256)
        cus, mem = C.c_int32(), C.c_int64()
        self._check(self._lib.ke_device_info(self._h, name, 256, C.byref(cus), C.byref(mem)), "ke_device_info")
        return {"name": name.value.decode(), "compute_units": cus.value, "total_mem": mem.value}

    def malloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._check(self._lib.ke_malloc(self._h, nbytes, C.byref(p)), "ke_malloc")
        return int(p.value)

    def free(self, ptr: int) -> None:
        self._check(self._lib.ke_free(self._h, ptr), "ke_free")

    def memcpy(self, dst, src, nbytes: int) -> None:
        self._check(self._lib.ke_memcpy(self._h, _addr(dst), _addr(src), nbytes), "ke_memcpy")

    def last_kernel_ms(self, kind: int) -> float:
        return float(self._lib.ke_last_kernel_ms(self._h, kind))

    def last_decode_sub_batches(self) -> int:
        """Sub-batches of the last decode call that ran the shared sub-batch loop (every kind but bmp and tiff, which have no scratch)."""
        return int(self._lib.ke_last_decode_sub_batches(self._h))

    def jpeg_last_split(self) -> tuple:
        """(files, lanes) of the last JPEG decode call on this context: the files whose restart intervals were decoded on lanes of
        their own (KE_JPEG_SPLIT_RESTARTS=1; the rule is in include/keyes.h) and the lanes launched for them.  (0, 0) with the
        variable unset."""
        files, lanes = C.c_int64(), C.c_int64()
        self._check(self._lib.ke_jpeg_last_split(self._h, C.byref(files), C.byref(lanes)), "ke_jpeg_last_split")
        return int(files.value), int(lanes.value)

    def last_scan_path(self) -> int:
        """Path the last hamming_scan with n >= 2 took, chosen on the device: 0 = all-pairs tiles, 1 = band buckets."""
        return int(self._lib.ke_last_scan_path(self._h))

    def last_resize_plan(self) -> tuple:
        """What the last group of the general resampler (resize_luma_uniform, fit_luma_uniform, the fit step of ssim_pairs, the
        thumbnail calls) was launched as: (banded, chunks per output, dwords per chunk, horizontal launches, bands per image,
        funnel-shift loader, vertical taps on the matrix cores, vertical pass first); -1 where an entry does not apply and
        before any call (include/keyes.h: ke_last_resize_plan)."""
        plan = np.empty(8, np.int32)
        self._check(self._lib.ke_last_resize_plan(self._h, _addr(plan)), "ke_last_resize_plan")
        return tuple(int(v) for v in plan)

    def last_ssim_plan(self) -> tuple:
        """What the last SSIM launch (ssim_pairs_uniform, or the last common size of the four pair calls) ran as: (kernel: 0 NaN
        fill, 1 exact, 2 fast; pixels per lane; aligned loader; column blocks; columns per block; rows per band; bands; why the
        loader: 0 aligned, 1 width, 2 base, 3 blocks); -1 where an entry does not apply and before any call (include/keyes.h:
        ke_last_ssim_plan)."""
        plan = np.empty(8, np.int32)
        self._check(self._lib.ke_last_ssim_plan(self._h, _addr(plan)), "ke_last_ssim_plan")
        return tuple(int(v) for v in plan)

    # -- hashing ----------------------------------------------------------------------------
    def hash_uniform(self, pixels, n: int, width: int, height: int, channels: int, *, want_phash=True,
                     want_dhash=True, phash_out=None, dhash_out=None, margin_out=None):
        """pixels: host ndarray (n,h,w[,c]) u8 or a device pointer.  Returns (phash u64[n] | None, dhash | None)
        as host arrays unless explicit output buffers (host arrays or device pointers) are given.
        margin_out: float32[n] host array or device pointer that receives the pHash tie margins (ke_hash_uniform_ex)."""
        if isinstance(pixels, np.ndarray):
            pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
            if pixels.size != n * width * height * channels:
                raise ValueError("pixel buffer does not match n*h*w*c")
        ph = phash_out if phash_out is not None else (np.empty(n, np.uint64) if want_phash else None)
        dh = dhash_out if dhash_out is not None else (np.empty(n, np.uint64) if want_dhash else None)
        with self._lock:
            if margin_out is not None:
                self._check(self._lib.ke_hash_uniform_ex(self._h, _addr(pixels), n, width, height, channels, _addr(ph),
                                                         _addr(dh), _addr(margin_out)), "ke_hash_uniform_ex")
            else:
                self._check(self._lib.ke_hash_uniform(self._h, _addr(pixels), n, width, height, channels, _addr(ph),
                                                      _addr(dh)), "ke_hash_uniform")
        return ph, dh

    def luma_tiles_uniform(self, pixels, n: int, width: int, height: int, channels: int, *, want32=True, want98=True):
        if isinstance(pixels, np.ndarray):
            pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
        t32 = np.empty((n, 32, 32), np.uint8) if want32 else None
        t98 = np.empty((n, 8, 9), np.uint8) if want98 else None
        with self._lock:
            self._check(self._lib.ke_luma_tiles_uniform(self._h, _addr(pixels), n, width, height, channels, _addr(t32),
                                                        _addr(t98)), "ke_luma_tiles_uniform")
        return t32, t98

    def hash_images(self, images: Sequence[np.ndarray], *, want_dhash=True, want_margin=False):
        """Ragged batch of host images sharing one channel count.  Returns (phash, dhash|None, status), plus the
        float32 tie margins as a fourth item with ``want_margin``."""
        n = len(images)
        if n == 0:
            return np.empty(0, np.uint64), (np.empty(0, np.uint64) if want_dhash else None), np.empty(0, np.int32)
        flat, offsets, widths, heights, ch = _pack_images(images)
        ph = np.empty(n, np.uint64)
        dh = np.empty(n, np.uint64) if want_dhash else None
        status = np.empty(n, np.int32)
        margin = np.empty(n, np.float32) if want_margin else None
        with self._lock:
            self._check(self._lib.ke_hash_images_ex(self._h, _addr(flat), _addr(offsets), _addr(widths), _addr(heights), ch, n,
                                                    _addr(ph), _addr(dh), _addr(status), _addr(margin)), "ke_hash_images_ex")
        return (ph, dh, status, margin) if want_margin else (ph, dh, status)

    def tiles_turned(self, tiles, n: Optional[int] = None):
        """The eight turned pHashes (include/keyes.h, ke_tiles_turned) of n 32x32 uint8 tiles: u64[n, 8], column k =
        the pHash arithmetic on orientation k of the tile.  ``tiles``: a host array or, with ``n``, a device pointer."""
        if isinstance(tiles, np.ndarray):
            tiles = np.ascontiguousarray(tiles, dtype=np.uint8)
            if tiles.size % 1024:
                raise ValueError("tiles must be 32 x 32 bytes each")
            n = tiles.size // 1024
        out = np.zeros((int(n), 8), np.uint64)
        with self._lock:
            self._check(self._lib.ke_tiles_turned(self._h, _addr(tiles), int(n), _addr(out)), "ke_tiles_turned")
        return out

    def _hash_views_at(self, mode: str, pixels, offsets, widths, heights, channels: int, tolerance: int = 0, *, leave=()) -> dict:
        """One call of HASH_CALLS[mode] on images that lie in one buffer -- a host array or a device pointer -- at any byte
        offsets: {output name: array, ..., "status": int32[n]} in the table's order, ``has`` as bool.  ``leave``: the outputs
        that are not wanted (the library gets a null pointer, the entry is None)."""
        name, takes_tolerance, outputs = HASH_CALLS[mode]
        offsets = np.ascontiguousarray(offsets, np.uint64)
        widths, heights = np.ascontiguousarray(widths, np.int32), np.ascontiguousarray(heights, np.int32)
        n = len(offsets)
        out = {key: None if key in leave else np.zeros((n,) + shape, dtype) for key, shape, dtype in outputs}
        out["status"] = np.zeros(n, np.int32)
        with self._lock:
            self._check(getattr(self._lib, name)(self._h, _addr(pixels), _addr(offsets), _addr(widths), _addr(heights), int(channels), n,
                                                 *((int(tolerance),) if takes_tolerance else ()), *(_addr(a) for a in out.values())), name)
        if out.get("has") is not None:
            out["has"] = out["has"].astype(bool)
        return out

    def _hash_views(self, mode: str, images: Sequence[np.ndarray], tolerance: int = 0) -> tuple:
        """``_hash_views_at`` of a ragged batch of host images sharing one channel count: the outputs, then the status."""
        if len(images) == 0:
            return tuple(hash_outputs(mode, 0).values())
        return tuple(self._hash_views_at(mode, *_pack_images(images), tolerance).values())

    def hash_images_turned(self, images: Sequence[np.ndarray]):
        """``hash_images`` with the eight turned pHashes in place of the two hashes: (turned u64[n, 8], status).  Column 0
        is the image's pHash; a failed image has eight zeros."""
        return self._hash_views("turned", images)

    def content_boxes(self, images: Sequence[np.ndarray], tolerance: int):
        """The content boxes (include/keyes.h, ke_content_boxes) of host images sharing one channel count:
        (boxes int32[n, 4] as (x0, y0, x1, y1), four zeros for an image without a box; status int32[n])."""
        n = len(images)
        if n == 0:
            return np.zeros((0, 4), np.int32), np.zeros(0, np.int32)
        flat, offsets, widths, heights, ch = _pack_images(images)
        boxes = np.zeros((n, 4), np.int32)
        status = np.zeros(n, np.int32)
        with self._lock:
            self._check(self._lib.ke_content_boxes(self._h, _addr(flat), _addr(offsets), _addr(widths), _addr(heights), ch, n, int(tolerance),
                                                   _addr(boxes), _addr(status)), "ke_content_boxes")
        return boxes, status

    def content_boxes_at(self, pixels, offsets, widths, heights, channels: int, tolerance: int):
        """``content_boxes`` of images that lie in one buffer already -- a host array or a device pointer -- at any byte
        offsets: (boxes int32[n, 4], status int32[n])."""
        offsets = np.ascontiguousarray(offsets, np.uint64)
        widths, heights = np.ascontiguousarray(widths, np.int32), np.ascontiguousarray(heights, np.int32)
        n = len(offsets)
        boxes = np.zeros((n, 4), np.int32)
        status = np.zeros(n, np.int32)
        with self._lock:
            self._check(self._lib.ke_content_boxes(self._h, _addr(pixels), _addr(offsets), _addr(widths), _addr(heights), int(channels), n,
                                                   int(tolerance), _addr(boxes), _addr(status)), "ke_content_boxes")
        return boxes, status

    def crop_pack(self, src: int, src_offsets, widths, heights, channels: int, boxes, dst: int, dst_offsets) -> None:
        """Rows [y0, y1) x columns [x0, x1) of image i of a device buffer (``boxes[i]``) -> ``dst + dst_offsets[i]`` of the
        caller's device buffer, rows packed (ke_crop_pack)."""
        so, do = np.ascontiguousarray(src_offsets, np.uint64), np.ascontiguousarray(dst_offsets, np.uint64)
        w, h = np.ascontiguousarray(widths, np.int32), np.ascontiguousarray(heights, np.int32)
        b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        if not len(so) == len(do) == len(w) == len(h) == len(b):
            raise ValueError("crop_pack: the arrays differ in length")
        with self._lock:
            self._check(self._lib.ke_crop_pack(self._h, src, _addr(so), _addr(w), _addr(h), int(channels), _addr(b), len(so), dst, _addr(do)),
                        "ke_crop_pack")

    def content_boxes_on_device(self, pointers, widths, heights, channels: int, tolerance: int):
        """``content_boxes`` of images that already lie in device memory, each at its own address (decoded there, or
        uploaded), as ``ssim_pairs_on_device`` takes them: (boxes int32[n, 4], status int32[n])."""
        ptrs = np.asarray(pointers, np.uint64)
        if len(ptrs) == 0:
            return np.zeros((0, 4), np.int32), np.zeros(0, np.int32)
        base = int(ptrs.min())
        return self.content_boxes_at(base, ptrs - np.uint64(base), widths, heights, channels, tolerance)

    def crop_luma(self, src: int, src_offsets, widths, heights, channels, boxes, dst: int, dst_offsets) -> None:
        """The ``convert("L")`` luma of rows [y0, y1) x columns [x0, x1) of image i of a device buffer (``boxes[i]``;
        ``channels[i]`` = 1, 3 or 4) -> ``dst + dst_offsets[i]`` of the caller's device buffer, one byte per pixel, rows packed
        (ke_crop_luma)."""
        so, do = np.ascontiguousarray(src_offsets, np.uint64), np.ascontiguousarray(dst_offsets, np.uint64)
        w, h = np.ascontiguousarray(widths, np.int32), np.ascontiguousarray(heights, np.int32)
        c = np.ascontiguousarray(channels, np.int32)
        b = np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        if not len(so) == len(do) == len(w) == len(h) == len(c) == len(b):
            raise ValueError("crop_luma: the arrays differ in length")
        with self._lock:
            self._check(self._lib.ke_crop_luma(self._h, src, _addr(so), _addr(w), _addr(h), _addr(c), _addr(b), len(so), dst, _addr(do)),
                        "ke_crop_luma")

    def hash_images_trimmed(self, images: Sequence[np.ndarray], tolerance: int):
        """``hash_images`` with the trimmed pHash (include/keyes.h, ke_hash_images_trimmed): (phash u64[n], boxes int32[n, 4],
        has bool[n], status int32[n]).  An image without a qualifying box has has = False and hash 0; its box is still there."""
        return self._hash_views("trimmed", images, tolerance)

    def hash_images_turned_trimmed(self, images: Sequence[np.ndarray], tolerance: int):
        """``hash_images_turned`` and ``hash_images_trimmed`` in one call, with the turned pHashes of the crop
        (ke_hash_images_turned_trimmed): (turned u64[n, 8], trimmed_turned u64[n, 8], boxes int32[n, 4], has bool[n], status
        int32[n]).  Column 0 of ``trimmed_turned`` is the trimmed pHash; a row is zeros where the box does not qualify."""
        return self._hash_views("turned_trimmed", images, tolerance)

    def hash_images_turned_trimmed_at(self, pixels, offsets, widths, heights, channels: int, tolerance: int):
        """``hash_images_turned_trimmed`` of images that lie in one buffer already -- a host array or a device pointer -- at any
        byte offsets."""
        return tuple(self._hash_views_at("turned_trimmed", pixels, offsets, widths, heights, channels, tolerance).values())

    # -- pinned staging ---------------------------------------------------------------------
    def stage_create(self, bytes_per_buffer: int, max_images: int, n_buffers: int = 2) -> None:
        self._stage_geom = None                              # whoever cached "my buffers are in place" (fastsig) must look again
        self._check(self._lib.ke_stage_create(self._h, int(bytes_per_buffer), int(max_images), int(n_buffers)), "ke_stage_create")

    def stage_create_shared(self, addresses, bytes_per_buffer: int, max_images: int) -> None:
        """Staging on the caller's page-aligned buffers (shared memory that decoder processes write into)."""
        ptrs = (C.c_void_p * len(addresses))(*[int(a) for a in addresses])
        self._stage_geom = None
        self._check(self._lib.ke_stage_create_shared(self._h, ptrs, int(bytes_per_buffer), int(max_images), len(addresses)),
                    "ke_stage_create_shared")

    def stage_destroy(self) -> None:
        self._stage_geom = None
        self._check(self._lib.ke_stage_destroy(self._h), "ke_stage_destroy")

    def stage_acquire(self):
        """Next pinned buffer in rotation: (slot, uint8 ndarray view of the whole buffer).  Blocks until the buffer's
        previous batch is done (its results land in the arrays given at its submit)."""
        slot, ptr, size = C.c_int32(), C.c_void_p(), C.c_size_t()
        with self._lock:
            self._check(self._lib.ke_stage_acquire(self._h, C.byref(slot), C.byref(ptr), C.byref(size)), "ke_stage_acquire")
        view = np.ctypeslib.as_array((C.c_uint8 * size.value).from_address(ptr.value))
        return int(slot.value), view

    def stage_submit_hash(self, slot: int, offsets, widths, heights, channels, *, want_dhash=True, want_margin=False):
        """Enqueue copy + hash of the images described; returns a dict of host arrays (phash, dhash, status, margin) that
        are valid after ``stage_wait(slot)`` (status: immediately).  The arrays must be kept alive until then."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        widths = np.ascontiguousarray(widths, dtype=np.int32)
        heights = np.ascontiguousarray(heights, dtype=np.int32)
        channels = np.ascontiguousarray(channels, dtype=np.int32)
        n = len(offsets)
        out = {"phash": np.zeros(n, np.uint64), "dhash": np.zeros(n, np.uint64) if want_dhash else None,
               "status": np.zeros(n, np.int32), "margin": np.zeros(n, np.float32) if want_margin else None,
               "_keep": (offsets, widths, heights, channels)}
        with self._lock:
            self._check(self._lib.ke_stage_submit_hash(self._h, slot, _addr(offsets), _addr(widths), _addr(heights), _addr(channels), n,
                                                       _addr(out["phash"]), _addr(out["dhash"]), _addr(out["status"]),
                                                       _addr(out["margin"])), "ke_stage_submit_hash")
        return out

    def stage_wait(self, slot: int = -1) -> None:
        with self._lock:
            self._check(self._lib.ke_stage_wait(self._h, int(slot)), "ke_stage_wait")

    # -- RCCL exchange ----------------------------------------------------------------------
    def comm_create(self, unique_id: bytes, world: int, rank: int) -> int:
        """ncclCommInitRank on this context's device; ``unique_id``: the 128 bytes of ``comm_unique_id()`` of rank 0."""
        comm = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._check(self._lib.ke_comm_create(self._h, buf, world, rank, C.byref(comm)), "ke_comm_create")
        return int(comm.value)

    def comm_destroy(self, comm: int) -> None:
        self._check(self._lib.ke_comm_destroy(self._h, comm), "ke_comm_destroy")

    def allgather_hashes(self, comm: int, world: int, local, n_total: int, table) -> None:
        """local: device pointer to ceil(n_total/world) u64; table: device pointer to n_total u64 (corpus order)."""
        self._check(self._lib.ke_allgather_hashes(self._h, comm, world, _addr(local), n_total, _addr(table)), "ke_allgather_hashes")

    def interleave_shards(self, gathered, world: int, n_total: int, table) -> None:
        self._check(self._lib.ke_interleave_shards(self._h, _addr(gathered), world, n_total, _addr(table)), "ke_interleave_shards")

    def allgather_edges(self, comm: int, world: int, local, n_local: int):
        """local: device pointer to this rank's ke_edge records.  Returns (all edges of all ranks as a host array, counts)."""
        counts = np.zeros(world, np.int64)
        total = C.c_int64(0)
        cap = max(1024, 2 * int(n_local) * world)
        while True:
            merged = np.empty(cap, EDGE_DTYPE)
            self._check(self._lib.ke_allgather_edges(self._h, comm, world, _addr(local), n_local, _addr(merged), cap, C.byref(total),
                                                     _addr(counts)), "ke_allgather_edges")
            if total.value <= cap:
                return merged[: total.value], counts
            cap = int(total.value)

    # -- file decode on the GPU (formats.FORMATS) ----------------------------------------------
    def _grow_host(self, buf: list, total: int) -> None:
        """A page-locked buffer ``[ptr, capacity, ...]`` made to hold ``total`` bytes (what it held is not kept)."""
        if total > buf[1]:
            if buf[0]:
                self._check(self._lib.ke_host_free(self._h, buf[0]), "ke_host_free")
                buf[0], buf[1] = 0, 0
            cap = max(total + total // 4, 1 << 24)
            p = C.c_void_p()
            self._check(self._lib.ke_host_alloc(self._h, cap, C.byref(p)), "ke_host_alloc")
            buf[0], buf[1] = int(p.value), cap

    def _packed(self, blobs, pinned: bool = True) -> _Files:
        """Files given as bytes, back to back in the context's page-locked buffer (grown on demand, reused from call to call):
        the copy to the device then runs at link speed.  Call with the lock held; the buffer is busy until the decode has
        returned.  ``pinned=False``: in an array of their own instead (a probe alone copies nothing to the device)."""
        n = len(blobs)
        sizes = np.fromiter((len(b) for b in blobs), np.uint64, n)
        offsets = np.zeros(n, np.uint64)
        offsets[1:] = np.cumsum(sizes[:-1])
        if not pinned:
            return _Files(np.frombuffer(b"".join(blobs) + bytes(64), np.uint8), offsets, sizes)     # one C-level copy; any alignment will do
        total = int(sizes.sum()) + 64
        if total > self.pack_limit and n > 1:
            raise _BatchTooLarge
        self._grow_host(self._pack, total)
        base = self._pack[0]
        srcs = (C.c_char_p * n)(*blobs)                    # the buffers of the bytes objects themselves, no copies
        if self._lib.ke_host_pack(base, srcs, _addr(offsets), _addr(sizes), n) != KE_OK:
            raise ValueError("ke_host_pack: bad arguments")
        C.memset(base + total - 64, 0, 64)
        return _Files(np.ctypeslib.as_array((C.c_uint8 * total).from_address(base)), offsets, sizes)

    def _read_files_into(self, buf: list, paths, bounded: bool = True) -> _Files:
        """The files themselves, read by the library's host threads straight into the page-locked buffer ``buf`` (no bytes
        objects, no interpreter loop over the files), which is grown when the batch needs it; unreadable files get size 0.
        ``bounded``: a batch of more than ``pack_limit`` bytes is _BatchTooLarge.  Nothing but ``buf`` is touched: call with the
        lock held when ``buf`` is the packing buffer (the read-ahead buffers have their own ``taken`` flag instead)."""
        n = len(paths)
        names = (C.c_char_p * n)(*[os.fsencode(p) for p in paths])
        offsets, sizes = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        needed = C.c_uint64(0)

        def read():
            return self._lib.ke_host_read_files(names, n, buf[0], buf[1], _addr(offsets), _addr(sizes), C.byref(needed))

        rc = read()
        if rc == -4:                                       # KE_ENOMEM: the buffer is too small for this batch
            if bounded and int(needed.value) > self.pack_limit and n > 1:
                raise _BatchTooLarge
            self._grow_host(buf, int(needed.value))
            rc = read()
        if rc != KE_OK:
            raise ValueError("ke_host_read_files: bad arguments")
        return _Files(np.ctypeslib.as_array((C.c_uint8 * int(needed.value)).from_address(buf[0])), offsets, sizes)

    def read_files_ahead(self, paths, spans=()):
        """Read files into one of the context's two page-locked read-ahead buffers -- from any thread, while another call of the
        context is decoding the previous batch on the GPU (nothing here touches the stream or the context's lock).  Returns a
        FilesAhead to pass to ``hash(..., ahead=(it, lo, hi))`` and to ``release()`` afterwards, or None when both buffers
        are taken or the files exceed ``pack_limit`` (the caller then lets the decode call read them itself).  ``spans`` =
        [(kind, lo, hi)]: the headers of files lo..hi are parsed here as well (``ke_<kind>_probe``), off the decoding thread."""
        paths = list(paths)
        if not paths:
            return None
        with self._ahead_lock:
            slot = next((k for k, buf in enumerate(self._ahead) if not buf[2]), None)
            if slot is None:
                return None
            self._ahead[slot][2] = True
        buf = self._ahead[slot]
        try:
            held = FilesAhead(self, slot, self._read_files_into(buf, paths))
        except _BatchTooLarge:
            buf[2] = False
            return None
        except BaseException:
            buf[2] = False
            raise
        for kind, lo, hi in spans:
            if hi > lo:
                try:
                    held.probed[(kind, lo, hi)] = self._probe(held.part(lo, hi), kind)
                except ValueError:
                    pass                                   # the decode call will say so
        return held

    def _probe(self, files: _Files, kind: str):
        """(widths, heights, channels, status) of packed files: ``ke_<kind>_probe`` (host code), or what the reader of a batch
        read ahead has parsed already."""
        n = len(files)
        known = files.probed.get((kind, files._first, files._first + n))
        if known is not None:
            return tuple(a.copy() for a in known)
        w, h, c, st = (np.zeros(n, np.int32) for _ in range(4))
        if getattr(self._lib, f"ke_{kind}_probe")(_addr(files.flat), _addr(files.offsets), _addr(files.sizes), n,
                                                  _addr(w), _addr(h), _addr(c), _addr(st)) != KE_OK:
            raise ValueError(f"ke_{kind}_probe: bad arguments")
        return w, h, c, st

    def probe(self, blobs, kind: str):
        """(widths, heights, channels, status) of files of a ``kind`` of formats.FORMATS given as bytes; status 0 = the GPU
        decoder takes the file."""
        return self._probe(self._packed(blobs, pinned=False), kind)

    def _decode_packed(self, files: _Files, kind: str, *, skip=None, owned: bool = False, by_shape: bool = False, denoms=None):
        """The one decode chain: probe -> bombs left to Pillow -> ``skip`` -> layout -> ``ke_<kind>_decode``, for what the GPU
        decoder takes of ``files``: (device ptr or 0, byte offsets, widths, heights, channels, status, caveat flags or None).
        ``denoms`` (JPEG only; int32 per file, or a function of the probed (widths, heights) that gives them): the files are
        decoded at 1 / denoms[i] by ``ke_jpeg_decode_scaled``, the widths and heights returned are those of the reduced images,
        and the denominators come back as an eighth item.
        The pixels go to the context's decode buffer (device memory, grown on demand and kept: allocating tens of GB per call
        costs up to a second) -- call with the lock held and keep it until they have been used; a batch of more than
        ``decode_limit`` bytes of them is _BatchTooLarge -- or, ``owned``, to an allocation the caller frees, laid out
        ``by_shape`` if asked (lay_out's groups of one (width, height, channels)), with the files' ``ke_<kind>_caveats``."""
        n = len(files)
        with self._lock:
            w, h, c, st = self._probe(files, kind)
            flags = np.zeros(n, np.int32) if owned else None
            if owned and getattr(self._lib, f"ke_{kind}_caveats")(_addr(files.flat), _addr(files.offsets), _addr(files.sizes), n, _addr(flags)) != KE_OK:
                raise ValueError(f"ke_{kind}_caveats: bad arguments")
            _leave_bombs_to_pillow(w, h, st, files.sizes)
            if skip is not None:                         # files the caller keeps for another decoder: as if refused
                skip = np.asarray(skip, bool)
                st[skip & (st == 0)] = 1
                files.sizes[skip] = 0
                left_alone = st[skip]
            if denoms is not None:
                if kind != "jpeg":
                    raise ValueError("only the jpeg decoder decodes at a reduced size")
                denoms = np.ascontiguousarray(denoms(w, h) if callable(denoms) else denoms, dtype=np.int32)
                if len(denoms) != n or not np.isin(denoms, (1, 2, 4, 8)).all():
                    raise ValueError("one denominator of 1, 2, 4 or 8 per file")
                w, h = ((w + denoms - 1) // denoms).astype(np.int32), ((h + denoms - 1) // denoms).astype(np.int32)
            nbytes = np.where(st == 0, w.astype(np.int64) * h * c, 0)
            out_off, total = lay_out(nbytes, (w, h, c), st != 0) if by_shape else lay_out(nbytes)     # decodable files first
            scaled = () if denoms is None else (denoms,)
            if total == 0:
                return (0, out_off, w, h, c, st, flags) + scaled
            if owned:
                dev = self.malloc(total + 64)
            else:
                if total > self.decode_limit and n > 1:
                    raise _BatchTooLarge
                if total + 64 > self._decoded_cap:
                    if self._decoded_ptr:
                        self.free(self._decoded_ptr)
                        self._decoded_ptr, self._decoded_cap = 0, 0
                    cap = total + total // 8 + 64
                    self._decoded_ptr, self._decoded_cap = self.malloc(cap), cap
                dev = self._decoded_ptr
            try:
                if denoms is not None:
                    self._check(self._lib.ke_jpeg_decode_scaled(self._h, _addr(files.flat), _addr(files.offsets), _addr(files.sizes), n,
                                                                _addr(denoms), dev, _addr(out_off), _addr(st)), "ke_jpeg_decode_scaled")
                else:
                    self._check(getattr(self._lib, f"ke_{kind}_decode")(self._h, _addr(files.flat), _addr(files.offsets), _addr(files.sizes), n,
                                                                        dev, _addr(out_off), _addr(st)), f"ke_{kind}_decode")
            except Exception:
                if owned:
                    self.free(dev)
                raise
            if skip is not None:                         # the decoder's word on a hidden file is its word on an empty one
                st[skip] = left_alone
            if not owned:
                self.decode_kernel_ms += self.last_kernel_ms(4)
        return (dev, out_off, w, h, c, st, flags) + scaled

    def decode_files_owned(self, paths, kind: str = "jpeg", *, by_shape: bool = False, draft_side: Optional[int] = None):
        """Files on disk decoded into a device buffer of their own (the caller frees it with ``free``): (device ptr or 0, byte
        offsets, widths, heights, channels, status, caveat flags).  ``flags`` are ke_jpeg_caveats / ke_png_caveats' bits: what
        the reference's defensive loader would do to the file beyond Image.open (EXIF orientation, transparency).
        ``by_shape``: images of one (width, height, channels) lie back to back without padding, so that each such group
        can go to the uniform-batch kernels as it is (runs_laid_out gives the groups back); files not decoded get NOT_LAID.
        ``draft_side`` (JPEG files): each file is decoded at the scale the loader's ``draft`` towards that side picks
        (``draft_scale``), the widths and heights are those of the reduced images, and the denominators follow as an eighth item."""
        paths = list(paths)
        if not paths:
            return (0, np.zeros(0, np.uint64)) + tuple(np.zeros(0, np.int32) for _ in range(5 if draft_side is None else 6))
        denoms = None if draft_side is None else (lambda w, h: draft_scale(w, h, draft_side))
        with self._lock:
            files = self._read_files_into(self._pack, paths, bounded=False)     # the caller paces its batches
            return self._decode_packed(files, kind, owned=True, by_shape=by_shape, denoms=denoms)

    def normalise_rgb(self, src: int, src_offsets, widths, heights, channels, orientations, *, by_shape: bool = False):
        """Images on the device (decoded files) -> a device buffer of their own (the caller frees it) holding them as the
        reference's loader would hand them over: turned by their EXIF orientation, RGBA composited over white
        (ke_normalise_rgb).  Returns (device ptr, byte offsets, widths, heights) of the RGB results, in input order;
        ``by_shape``: results of one (width, height) lie back to back without padding (a group starts on 16 bytes), so that
        each group can go to the uniform-batch kernels as it is."""
        so = np.ascontiguousarray(src_offsets, dtype=np.uint64)
        w, h = np.ascontiguousarray(widths, dtype=np.int32), np.ascontiguousarray(heights, dtype=np.int32)
        c, o = np.ascontiguousarray(channels, dtype=np.int32), np.ascontiguousarray(orientations, dtype=np.int32)
        n = len(so)
        turned = o >= 5
        ow, oh = np.where(turned, h, w).astype(np.int32), np.where(turned, w, h).astype(np.int32)
        nbytes = ow.astype(np.int64) * oh * 3
        do, total = lay_out(nbytes, (oh, ow)) if by_shape else lay_out(nbytes)
        dev = self.malloc(total + 64)
        try:
            with self._lock:
                self._check(self._lib.ke_normalise_rgb(self._h, src, _addr(so), _addr(w), _addr(h), _addr(c), _addr(o), n, dev, _addr(do)),
                            "ke_normalise_rgb")
        except Exception:
            self.free(dev)
            raise
        return dev, do, ow, oh

    def thumbnail_rgb(self, src: int, width: int, height: int, box: int, filter: int = 0):
        """An RGB image on the device -> what ``Image.thumbnail((box, box), LANCZOS)`` makes of it, in a device buffer of its own
        (the caller frees it): (device ptr, width, height).  The size is Image.thumbnail's (aspect preserved, PIL/Image.py
        ``preserve_aspect_ratio``); ke_thumbnail_rgb resamples each band as Pillow does."""
        x, y = thumbnail_size(width, height, box)
        dev = self.malloc(x * y * 3 + 64)
        try:
            with self._lock:
                self._check(self._lib.ke_thumbnail_rgb(self._h, src, width, height, x, y, filter, dev), "ke_thumbnail_rgb")
        except Exception:
            self.free(dev)
            raise
        return dev, x, y

    def reduce_rgb(self, src: int, width: int, height: int, fx: int, fy: int):
        """An RGB image on the device -> ``Image.reduce((fx, fy))`` of it in a device buffer of its own (the caller frees it):
        (device ptr, width, height) -- ke_reduce_rgb, factors 1..255 per axis."""
        ow, oh = -(-width // fx), -(-height // fy)
        dev = self.malloc(ow * oh * 3 + 64)
        try:
            with self._lock:
                self._check(self._lib.ke_reduce_rgb(self._h, src, width, height, fx, fy, dev), "ke_reduce_rgb")
        except Exception:
            self.free(dev)
            raise
        return dev, ow, oh

    def thumbnail_rgb_box(self, src: int, width: int, height: int, out_w: int, out_h: int, box, filter: int = 0):
        """An RGB image on the device resampled to out_w x out_h through the source rectangle ``box`` = (x0, y0, x1, y1), as
        ``Image.resize((out_w, out_h), filter, box=box)`` does, into a device buffer of its own (the caller frees it)."""
        box = np.ascontiguousarray(box, dtype=np.float32)
        dev = self.malloc(out_w * out_h * 3 + 64)
        try:
            with self._lock:
                self._check(self._lib.ke_thumbnail_rgb_box(self._h, src, width, height, out_w, out_h, filter, _addr(box), dev),
                            "ke_thumbnail_rgb_box")
        except Exception:
            self.free(dev)
            raise
        return dev

    def thumbnail_rgb_reduced(self, src: int, width: int, height: int, box: int):
        """``Image.thumbnail((box, box), LANCZOS)`` of an RGB image on the device of any size, with what Pillow's
        ``reducing_gap`` of 2.0 does to one more than four times its target: ``Image.reduce`` by (fx, fy) first, then the
        resample through the fractional source box (0, 0, width / fx, height / fy) of the reduced image.  Returns (device ptr
        -- the caller frees it --, width, height, (fx, fy)); with both factors 1 the result is ``thumbnail_rgb``'s."""
        x, y = thumbnail_size(width, height, box)
        fx, fy = int(width / x / 2.0) or 1, int(height / y / 2.0) or 1
        if fx == 1 and fy == 1:
            return self.thumbnail_rgb(src, width, height, box) + ((1, 1),)
        small, sw, sh = self.reduce_rgb(src, width, height, fx, fy)
        try:
            return self.thumbnail_rgb_box(small, sw, sh, x, y, (0.0, 0.0, width / fx, height / fy)), x, y, (fx, fy)
        finally:
            self.free(small)

    def jpeg_decode_scaled(self, blobs, denoms=None, *, max_side: Optional[int] = None):
        """JPEG files (bytes) decoded on the GPU at 1 / denoms[i] (1, 2, 4 or 8) -- the pixels Pillow yields after ``draft`` has
        set that scale up --, or, with ``max_side`` instead, at the scale the reference's loader drafts each file to
        (``draft_scale``).  Returns (list of ndarrays, None where status != 0; statuses; the denominators)."""
        if (denoms is None) == (max_side is None):
            raise ValueError("either denoms or max_side")
        with self._lock:
            dev, out_off, w, h, c, st, _, used = self._decode_packed(
                self._packed(blobs), "jpeg", denoms=denoms if denoms is not None else (lambda w, h: draft_scale(w, h, max_side)))
            out = [None] * len(blobs)
            for i in np.nonzero(st == 0)[0].tolist():
                out[i] = np.empty((h[i], w[i], c[i]) if c[i] > 1 else (h[i], w[i]), np.uint8)
                self.memcpy(out[i], dev + int(out_off[i]), out[i].nbytes)
        return out, st, used

    def release_decode_buffers(self) -> None:
        """Give back the page-locked packing buffer and the device decode buffer (they are kept between calls otherwise)."""
        with self._lock:
            if self._pack[0]:
                self._check(self._lib.ke_host_free(self._h, self._pack[0]), "ke_host_free")
                self._pack[0], self._pack[1] = 0, 0
            if self._decoded_ptr:
                self.free(self._decoded_ptr)
                self._decoded_ptr, self._decoded_cap = 0, 0
            with self._ahead_lock:
                for buf in self._ahead:
                    if buf[0] and not buf[2]:
                        self._check(self._lib.ke_host_free(self._h, buf[0]), "ke_host_free")
                        buf[0], buf[1] = 0, 0

    def decode(self, blobs, kind: str):
        """Pixels of files of a ``kind`` of formats.FORMATS decoded on the GPU: list of ndarrays (HxW or HxWxC, see the kind's
        row) with None where the decoder refused the file (status != 0); also returns the statuses."""
        def run(lo: int, hi: int):
            out = [None] * (hi - lo)
            dev, out_off, w, h, c, st, _ = self._decode_packed(self._packed(blobs[lo:hi]), kind)
            for i in np.nonzero(st == 0)[0].tolist():
                out[i] = np.empty((h[i], w[i], c[i]) if c[i] > 1 else (h[i], w[i]), np.uint8)
                self.memcpy(out[i], dev + int(out_off[i]), out[i].nbytes)
            return out, st

        with self._lock:                                 # the decode buffer is this call's until the pixels are out
            parts = _in_halves(run, 0, len(blobs))
        return [a for p in parts for a in p[0]], np.concatenate([p[1] for p in parts])

    def hash_files(self, paths, *, want_dhash=True, kind: str = "jpeg"):
        """``hash`` for files on disk: read (host threads, page-locked buffer), decoded and hashed on the GPU."""
        return self.hash(None, want_dhash=want_dhash, kind=kind, paths=list(paths))

    def hash(self, blobs, *, want_dhash=True, kind: str = "jpeg", paths=None, ahead=None, skip=None):
        """pHash / dHash of files of a ``kind`` of formats.FORMATS, decoded and hashed without the pixels leaving the GPU.
        Returns (phash u64[n], dhash u64[n] | None, status int32[n]); status != 0 = not handled here (decode the file with
        Pillow).  The files come as bytes (``blobs``), as ``paths`` the library reads, or as ``ahead = (FilesAhead, lo, hi)``:
        files lo..hi of a batch read beforehand.  ``skip``: a mask of files to leave alone (status 1)."""
        return tuple(self._hash_chain("plain", blobs, kind, paths, ahead, skip, leave=() if want_dhash else ("dhash",)).values())

    def hash_turned(self, blobs, *, kind: str, paths=None):
        """``hash``'s chain with ke_hash_images_turned behind the decode: (turned u64[n, 8], status int32[n]); status != 0 =
        not handled here, eight zeros."""
        return tuple(self._hash_chain("turned", blobs, kind, paths).values())

    def hash_trimmed(self, blobs, *, kind: str, paths=None, tolerance: int = 48):
        """``hash``'s chain with ke_hash_images_trimmed behind the decode: (phash u64[n], boxes int32[n, 4], has bool[n],
        status int32[n]); status != 0 = not handled here, zeros."""
        return tuple(self._hash_chain("trimmed", blobs, kind, paths, tolerance=tolerance).values())

    def hash_turned_trimmed(self, blobs, *, kind: str, paths=None, tolerance: int = 48):
        """``hash``'s chain with ke_hash_images_turned_trimmed behind the decode: (turned u64[n, 8], trimmed_turned u64[n, 8],
        boxes int32[n, 4], has bool[n], status int32[n]); status != 0 = not handled here, zeros."""
        return tuple(self._hash_chain("turned_trimmed", blobs, kind, paths, tolerance=tolerance).values())

    def _hash_chain(self, mode: str, blobs, kind, paths, ahead=None, skip=None, *, tolerance: int = 0, leave=()) -> dict:
        """Files decoded on the GPU and handed to HASH_CALLS[mode] there, channel count by channel count: ``hash_outputs`` of
        the mode over all the files, zeros and status != 0 for a file the decoder or the hash call refused."""
        if ahead is not None:                            # where the files come from is settled here, once
            n = ahead[2] - ahead[1]
            take = lambda lo, hi: ahead[0].part(ahead[1] + lo, ahead[1] + hi)
        elif paths is not None:
            n = len(paths)
            take = lambda lo, hi: self._read_files_into(self._pack, paths[lo:hi])
        else:
            n = len(blobs)
            take = lambda lo, hi: self._packed(blobs[lo:hi])
        if n == 0:
            return hash_outputs(mode, 0, leave)
        skip = None if skip is None else np.asarray(skip, bool)

        def run(lo: int, hi: int) -> dict:
            out = hash_outputs(mode, hi - lo, leave)
            dev, out_off, w, h, c, st, _ = self._decode_packed(take(lo, hi), kind, skip=None if skip is None else skip[lo:hi])
            for ch in (1, 3, 4):
                idx = np.nonzero((st == 0) & (c == ch))[0]
                if len(idx) == 0:
                    continue
                got = self._hash_views_at(mode, dev, out_off[idx], w[idx], h[idx], ch, tolerance, leave=leave)
                st[idx[got.pop("status") != 0]] = 2
                for name, values in got.items():
                    if values is not None:
                        out[name][idx] = values
            out["status"] = st
            return out

        with self._lock:                                 # the decode buffer is this call's until the pixels are hashed
            parts = _in_halves(run, 0, n)
        return {name: None if name in leave else np.concatenate([p[name] for p in parts]) for name in parts[0]}

    # -- scan -------------------------------------------------------------------------------
    def hamming_scan(self, hashes, n: int, *, ids=None, sizes=None, threshold=8, band_bits=16, band_count=4,
                     size_ratio: float = 0.0, bucket_pair_cap: int = 0, part_index=0, part_count=1,
                     capacity: Optional[int] = None, first_new: Optional[int] = None, cross: bool = False, exact: bool = False):
        """Returns (edges[EDGE_DTYPE] on the host, counters u64[4]).  hashes/ids/sizes: host arrays or device ptrs.
        first_new > 0: only the edges whose later position is at least first_new (ke_hamming_scan_from); counters[0] is
        then the region's pair count, [1] and [2] are over those edges, [3] stays the whole table's.
        cross=True (needs first_new): the table is [library | queries] and only the edges a < first_new <= b come back
        (ke_hamming_scan_cross); counters[0] is first_new * (n - first_new) over the shards.
        exact=True (ke_hamming_scan_exact): every pair of the same region -- all pairs, from first_new, or cross -- within the
        threshold, whether or not it shares a band; ``bands`` is 0 for a pair that shares none, so the edges with bands != 0 are
        the banded call's.  counters[3] is 0.  A bucket pair cap has no meaning there: ValueError with a non-zero one."""
        if cross and first_new is None:
            raise ValueError("cross=True needs first_new")
        if exact and int(bucket_pair_cap or 0) != 0:
            raise ValueError("exact=True takes no bucket_pair_cap: the cap is a property of buckets")
        first_new = int(first_new or 0)

        def host(a, dt):
            return np.ascontiguousarray(a, dtype=dt) if isinstance(a, (np.ndarray, list, tuple)) else a

        hashes, ids, sizes = host(hashes, np.uint64), host(ids, np.int64), host(sizes, np.int64)
        cap = int(capacity) if capacity else max(1 << 16, 2 * int(n))
        counters = np.zeros(4, np.uint64)
        n_edges = C.c_int64(0)
        # the four calls differ in what stands between n and the shard, and in whether they take a cap
        region = 2 if cross else 1 if first_new else 0
        if exact:
            name, after_n, pair_cap = "ke_hamming_scan_exact", (first_new, region), ()
        else:
            name, after_n = (("ke_hamming_scan", ()), ("ke_hamming_scan_from", (first_new,)), ("ke_hamming_scan_cross", (first_new,)))[region]
            pair_cap = (int(bucket_pair_cap),)
        while True:
            edges = np.empty(cap, EDGE_DTYPE)
            with self._lock:
                self._check(getattr(self._lib, name)(self._h, _addr(hashes), _addr(ids), _addr(sizes), n, *after_n, part_index,
                                                     part_count, threshold, band_bits, band_count, float(size_ratio), *pair_cap,
                                                     _addr(edges), cap, C.byref(n_edges), _addr(counters)), name)
            if n_edges.value <= cap:
                return edges[: n_edges.value], counters
            cap = int(n_edges.value)  # overflow protocol: retry with the reported size

    def hamming_nearest(self, hashes, queries, *, k: int, max_distance: int = 64, ids=None, query_ids=None, histogram: bool = False,
                        n: Optional[int] = None, m: Optional[int] = None):
        """The k nearest entries of ``hashes`` for every query, by Hamming distance alone (ke_hamming_nearest): row q holds the
        first min(k, |S_q|) of S_q = {i : popcount(hashes[i] ^ queries[q]) <= max_distance, ids[i] != query_ids[q] where both id
        arrays are given}, ordered by (distance, position).  No band predicate, no size filter, no bucket cap.
        Returns (index int64[m, k], distance int32[m, k], count int32[m], within int64[m]), -1 beyond count, and
        histogram uint32[m, 65] after them when asked.  Inputs: host arrays or device pointers; a device pointer needs its
        length in ``n`` (hashes, ids) or ``m`` (queries, query_ids)."""
        def host(a, dt):
            return np.ascontiguousarray(a, dtype=dt) if isinstance(a, (np.ndarray, list, tuple)) else a

        hashes, queries = host(hashes, np.uint64), host(queries, np.uint64)
        ids, query_ids = host(ids, np.int64), host(query_ids, np.int64)
        n = int(len(hashes) if n is None else n)
        m = int(len(queries) if m is None else m)
        for name, a, want in (("hashes", hashes, n), ("ids", ids, n), ("queries", queries, m), ("query_ids", query_ids, m)):
            if isinstance(a, np.ndarray) and a.size != want:
                raise ValueError(f"{name} has {a.size} entries, expected {want}")
        rows, width = max(m, 0), max(int(k), 0)
        index = np.full((rows, width), -1, np.int64)
        distance = np.full((rows, width), -1, np.int32)
        count = np.zeros(rows, np.int32)
        within = np.zeros(rows, np.int64)
        hist = np.zeros((rows, 65), np.uint32) if histogram else None
        with self._lock:
            self._check(self._lib.ke_hamming_nearest(self._h, _addr(hashes), _addr(ids), n, _addr(queries), _addr(query_ids), m,
                                                     int(k), int(max_distance), _addr(index), _addr(distance), _addr(count),
                                                     _addr(within), _addr(hist)), "ke_hamming_nearest")
        return (index, distance, count, within) + ((hist,) if histogram else ())

    def band_pairs_after_size(self, hashes, sizes, n: int, *, band_bits=16, band_count=4, size_ratio: float, bucket_pair_cap: int = 0) -> int:
        """The reference's "size=" funnel counter before pairs of equal file id are taken out (ke_band_pairs_after_size)."""
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64) if isinstance(hashes, np.ndarray) else hashes
        sizes = np.ascontiguousarray(sizes, dtype=np.int64) if isinstance(sizes, np.ndarray) else sizes
        out = np.zeros(1, np.uint64)
        with self._lock:
            self._check(self._lib.ke_band_pairs_after_size(self._h, _addr(hashes), _addr(sizes), n, band_bits, band_count,
                                                           float(size_ratio), int(bucket_pair_cap), _addr(out)), "ke_band_pairs_after_size")
        return int(out[0])

    def cluster_labels(self, edges: np.ndarray, n_nodes: int) -> np.ndarray:
        return cluster_labels(edges, n_nodes)

    # -- ssim -------------------------------------------------------------------------------
    def ssim_set_mode(self, exact: bool) -> None:
        """False (default): integer-sum kernel, within 1e-5 of skimage's float32 arithmetic; True: the kernel that
        reproduces every rounding (bit-identical to the oracle, 3-4x slower)."""
        self._check(self._lib.ke_ssim_set_mode(self._h, 1 if exact else 0), "ke_ssim_set_mode")

    def ssim_pairs_uniform(self, images, n_images: int, width: int, height: int, channels: int, pair_a, pair_b):
        if isinstance(images, np.ndarray):
            images = np.ascontiguousarray(images, dtype=np.uint8)
        pa = np.ascontiguousarray(pair_a, dtype=np.int64)
        pb = np.ascontiguousarray(pair_b, dtype=np.int64)
        out = np.empty(len(pa), np.float64)
        with self._lock:
            self._check(self._lib.ke_ssim_pairs_uniform(self._h, _addr(images), n_images, width, height, channels, _addr(pa),
                                                        _addr(pb), len(pa), _addr(out)), "ke_ssim_pairs_uniform")
        return out

    def _ssim_pairs_views(self, what: str, pixels, offsets, widths, heights, channels: int, pair_a, pair_b, box_a=None, box_b=None,
                          orient_b=None, plain: bool = False):
        """The four pair calls: ``pixels`` a host array or a base address, ``offsets`` from it.  One ``ke_ssim_pairs_viewed`` call
        (``plain``: ``ke_ssim_pairs``, which has neither boxes nor orientations) -> (float64 scores, int32 statuses)."""
        pa = np.ascontiguousarray(pair_a, dtype=np.int64)
        pb = np.ascontiguousarray(pair_b, dtype=np.int64)
        boxes = []
        for b in (box_a, box_b):
            b = None if b is None else np.ascontiguousarray(b, dtype=np.int32).reshape(-1, 4)
            if b is not None and len(b) != len(pa):
                raise ValueError(f"{what}: a box array holds one box per pair")
            boxes.append(b)
        ob = None if orient_b is None else np.ascontiguousarray(orient_b, dtype=np.int32)
        if len(pb) != len(pa) or (ob is not None and len(ob) != len(pa)):
            raise ValueError(f"{what}: the pair arrays differ in length")
        offsets = np.ascontiguousarray(offsets, np.uint64)
        widths = np.ascontiguousarray(widths, np.int32)
        heights = np.ascontiguousarray(heights, np.int32)
        out = np.empty(len(pa), np.float64)
        status = np.empty(len(pa), np.int32)
        head = (self._h, _addr(pixels), _addr(offsets), _addr(widths), _addr(heights), int(channels), len(widths), _addr(pa), _addr(pb))
        tail = (len(pa), _addr(out), _addr(status))
        with self._lock:
            if plain:
                self._check(self._lib.ke_ssim_pairs(*head, *tail), "ke_ssim_pairs")
            else:
                self._check(self._lib.ke_ssim_pairs_viewed(*head, _addr(boxes[0]), _addr(boxes[1]), _addr(ob), *tail), "ke_ssim_pairs_viewed")
        return out, status

    def ssim_pairs(self, images: Sequence[np.ndarray], pair_a, pair_b):
        """src/dup/refine.py:44-52 for pairs of images of any sizes (one channel count): common size, ImageOps.fit + BICUBIC
        of both, SSIM.  Returns (float64 scores, NaN where the status is not 0; int32 statuses KE_PAIR_*)."""
        return self._ssim_pairs_views("ssim_pairs", *_pack_images(images), pair_a, pair_b, plain=True)

    def ssim_pairs_on_device(self, pointers, widths, heights, channels: int, pair_a, pair_b):
        """ssim_pairs for images that already lie in device memory, each at its own address (decoded there, or uploaded)."""
        return self._ssim_pairs_views("ssim_pairs", *_base_and_offsets(pointers), widths, heights, channels, pair_a, pair_b, plain=True)

    def ssim_pairs_turned(self, images: Sequence[np.ndarray], pair_a, pair_b, orient_b):
        """ssim_pairs with image ``pair_b[k]`` under orientation ``orient_b[k]`` (0..7, turned.ORIENTATIONS; None: all 0)."""
        return self._ssim_pairs_views("ssim_pairs_turned", *_pack_images(images), pair_a, pair_b, None, None, orient_b)

    def ssim_pairs_turned_on_device(self, pointers, widths, heights, channels: int, pair_a, pair_b, orient_b):
        """ssim_pairs_on_device with image ``pair_b[k]`` under orientation ``orient_b[k]`` (0..7, turned.ORIENTATIONS): each
        distinct (image, orientation != 0) is turned once on the device (ke_turn_luma) before the fit."""
        return self._ssim_pairs_views("ssim_pairs_turned", *_base_and_offsets(pointers), widths, heights, channels, pair_a, pair_b, None, None,
                                      orient_b)

    def ssim_pairs_boxed(self, images: Sequence[np.ndarray], pair_a, pair_b, box_a, box_b):
        """ssim_pairs on boxes of the images (ke_ssim_pairs_boxed): pair k is box ``box_a[k]`` of image ``pair_a[k]`` against box
        ``box_b[k]`` of image ``pair_b[k]``, boxes as (x0, y0, x1, y1).  ``None``, four zeros and (0, 0, w, h) mean the image as it
        lies.  The scores are those of ``ssim_pairs`` on images that hold the crops, bit for bit."""
        return self._ssim_pairs_views("ssim_pairs_boxed", *_pack_images(images), pair_a, pair_b, box_a, box_b)

    def ssim_pairs_boxed_on_device(self, pointers, widths, heights, channels: int, pair_a, pair_b, box_a, box_b):
        """ssim_pairs_on_device on boxes of the images: each distinct (image, box) is cut out once on the device, luma only
        (ke_crop_luma), before the fit."""
        return self._ssim_pairs_views("ssim_pairs_boxed", *_base_and_offsets(pointers), widths, heights, channels, pair_a, pair_b, box_a, box_b)

    def ssim_pairs_viewed(self, images: Sequence[np.ndarray], pair_a, pair_b, box_a, box_b, orient_b):
        """ssim_pairs on views of the images (ke_ssim_pairs_viewed): pair k is box ``box_a[k]`` of image ``pair_a[k]`` against
        orientation ``orient_b[k]`` (0..7, turned.ORIENTATIONS; None: all 0) of box ``box_b[k]`` of image ``pair_b[k]`` -- crop,
        then turn, then fit.  Boxes as in ``ssim_pairs_boxed``.  The scores are those of ``ssim_pairs`` on images that hold
        ``turn(k, crop)``, bit for bit."""
        return self._ssim_pairs_views("ssim_pairs_viewed", *_pack_images(images), pair_a, pair_b, box_a, box_b, orient_b)

    def ssim_pairs_viewed_on_device(self, pointers, widths, heights, channels: int, pair_a, pair_b, box_a, box_b, orient_b):
        """ssim_pairs_on_device on views of the images: each distinct (image, box, orientation) is made once on the device, luma
        only (ke_crop_luma, ke_turn_luma or ke_crop_turn_luma), before the fit."""
        return self._ssim_pairs_views("ssim_pairs_viewed", *_base_and_offsets(pointers), widths, heights, channels, pair_a, pair_b, box_a,
                                      box_b, orient_b)

    def _view_luma(self, what: str, src: int, src_offsets, widths, heights, channels, boxes, orientations, dst: int, dst_offsets) -> None:
        """turn_luma (``boxes`` None: ke_turn_luma) and crop_turn_luma (ke_crop_turn_luma)."""
        so, do = np.ascontiguousarray(src_offsets, dtype=np.uint64), np.ascontiguousarray(dst_offsets, dtype=np.uint64)
        w, h = np.ascontiguousarray(widths, dtype=np.int32), np.ascontiguousarray(heights, dtype=np.int32)
        c, o = np.ascontiguousarray(channels, dtype=np.int32), np.ascontiguousarray(orientations, dtype=np.int32)
        b = None if boxes is None else np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
        if not len(so) == len(do) == len(w) == len(h) == len(c) == len(o) == (len(so) if b is None else len(b)):
            raise ValueError(f"{what}: the arrays differ in length")
        head, tail = (self._h, src, _addr(so), _addr(w), _addr(h), _addr(c)), (_addr(o), len(so), dst, _addr(do))
        with self._lock:
            if b is None:
                self._check(self._lib.ke_turn_luma(*head, *tail), "ke_turn_luma")
            else:
                self._check(self._lib.ke_crop_turn_luma(*head, _addr(b), *tail), "ke_crop_turn_luma")

    def crop_turn_luma(self, src: int, src_offsets, widths, heights, channels, boxes, orientations, dst: int, dst_offsets) -> None:
        """The ``convert("L")`` luma of orientation ``orientations[i]`` (0..7, turned.ORIENTATIONS) of box ``boxes[i]`` of image i of
        a device buffer -> ``dst + dst_offsets[i]`` of the caller's device buffer, one byte per pixel, rows packed, the box's
        sides swapped for k & 4 (ke_crop_turn_luma)."""
        self._view_luma("crop_turn_luma", src, src_offsets, widths, heights, channels, boxes, orientations, dst, dst_offsets)

    def turn_luma(self, src: int, src_offsets, widths, heights, channels, orientations, dst: int, dst_offsets) -> None:
        """Images on the device (``widths[i]`` x ``heights[i]``, 1, 3 or 4 channels, at ``src + src_offsets[i]``) -> the luma plane
        of orientation ``orientations[i]`` (0..7, turned.ORIENTATIONS) of each, one byte per pixel, rows packed, at
        ``dst + dst_offsets[i]`` of the caller's device buffer (ke_turn_luma): ``heights[i]`` x ``widths[i]`` for k & 4."""
        self._view_luma("turn_luma", src, src_offsets, widths, heights, channels, None, orientations, dst, dst_offsets)

    # -- shipped refine stage -------------------------------------------------------------------
    def resize_luma_uniform(self, pixels, n: int, width: int, height: int, channels: int, out_w: int, out_h: int,
                            filter: int = 1, out=None):
        """n images -> (n, out_h, out_w) u8 luma thumbnails; filter 0 = LANCZOS, 1 = BILINEAR."""
        if isinstance(pixels, np.ndarray):
            pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
        if out is None:
            out = np.empty((n, out_h, out_w), np.uint8)
        with self._lock:
            self._check(self._lib.ke_resize_luma_uniform(self._h, _addr(pixels), n, width, height, channels, out_w, out_h,
                                                         filter, _addr(out)), "ke_resize_luma_uniform")
        return out

    def fit_luma_uniform(self, pixels, n: int, width: int, height: int, channels: int, out_w: int, out_h: int,
                         filter: int = 2, out=None):
        """n images -> (n, out_h, out_w) u8: ImageOps.fit(image.convert("L"), (out_w, out_h), filter) of Pillow
        (centre crop to the aspect ratio + resize); filter 2 = BICUBIC as src/dup/refine.py:48 uses."""
        if isinstance(pixels, np.ndarray):
            pixels = np.ascontiguousarray(pixels, dtype=np.uint8)
        if out is None:
            out = np.empty((n, out_h, out_w), np.uint8)
        with self._lock:
            self._check(self._lib.ke_fit_luma_uniform(self._h, _addr(pixels), n, width, height, channels, out_w, out_h,
                                                      filter, _addr(out)), "ke_fit_luma_uniform")
        return out

    def tile_ahash(self, tiles, n: int, grid: int, tile: int):
        """(n, side, side) thumbnails -> (n, words) u64, little-endian bit order of tile_ahash_bits."""
        if isinstance(tiles, np.ndarray):
            tiles = np.ascontiguousarray(tiles, dtype=np.uint8)
        side = grid * tile
        words = (side * side + 63) // 64
        out = np.empty((n, words), np.uint64)
        with self._lock:
            self._check(self._lib.ke_tile_ahash(self._h, _addr(tiles), n, grid, tile, _addr(out)), "ke_tile_ahash")
        return out

    def sad_pairs(self, thumbs, n_thumbs: int, pixels: int, pair_a, pair_b):
        if isinstance(thumbs, np.ndarray):
            thumbs = np.ascontiguousarray(thumbs, dtype=np.uint8)
        pa = np.ascontiguousarray(pair_a, dtype=np.int64)
        pb = np.ascontiguousarray(pair_b, dtype=np.int64)
        out = np.empty(len(pa), np.uint64)
        with self._lock:
            self._check(self._lib.ke_sad_pairs(self._h, _addr(thumbs), n_thumbs, pixels, _addr(pa), _addr(pb), len(pa),
                                               _addr(out)), "ke_sad_pairs")
        return out

    # -- synthetic corpus ---------------------------------------------------------------------
    def synth_rgb(self, seed: int, first: int, n: int, width: int, height: int, out=None):
        if out is None:
            out = np.empty((n, height, width, 3), np.uint8)
        with self._lock:
            self._check(self._lib.ke_synth_rgb(self._h, seed, first, n, width, height, _addr(out)), "ke_synth_rgb")
        return out

    def synth_rgb_indexed(self, seed: int, indices, width: int, height: int, out: int) -> None:
        """Corpus images indices[k] -> device memory at ``out`` (k-th image at out + k*w*h*3)."""
        idx = np.ascontiguousarray(indices, dtype=np.int64)
        with self._lock:
            self._check(self._lib.ke_synth_rgb_indexed(self._h, seed, _addr(idx), len(idx), width, height, out), "ke_synth_rgb_indexed")

    def synth_hashes(self, seed: int, n: int, out=None):
        if out is None:
            out = np.empty(n, np.uint64)
        with self._lock:
            self._check(self._lib.ke_synth_hashes(self._h, seed, n, _addr(out)), "ke_synth_hashes")
        return out


def _name_per_kind(fmt) -> None:
    """``Context.<kind>_probe`` / ``_decode`` / ``_hash``: the generic calls under the names tests, benchmarks and
    INTEGRATION.md use (``kind=`` still overrides, as ``jpeg_hash(kind="png")`` always did)."""
    def probe(self, blobs, kind: str = fmt.kind):
        return self.probe(blobs, kind)

    def decode(self, blobs, kind: str = fmt.kind):
        return self.decode(blobs, kind)

    def hash_(self, blobs, *, want_dhash=True, kind: str = fmt.kind, paths=None, ahead=None, skip=None):
        return self.hash(blobs, want_dhash=want_dhash, kind=kind, paths=paths, ahead=ahead, skip=skip)

    probe.__doc__ = f"``probe`` of {fmt.kind} files: (widths, heights, channels, status); status 0 = the GPU decoder takes the file."
    decode.__doc__ = f"{fmt.decodes}, None where the decoder refused the file; and the per-file status."
    hash_.__doc__ = f"``hash`` of {fmt.kind} files: (phash, dhash | None, status); status != 0 = decode the file with Pillow."
    for call, fn in (("probe", probe), ("decode", decode), ("hash", hash_)):
        fn.__name__ = f"{fmt.kind}_{call}"
        fn.__qualname__ = f"Context.{fn.__name__}"
        setattr(Context, fn.__name__, fn)


for _fmt in FORMATS:
    _name_per_kind(_fmt)


_default: dict = {}
_default_lock = threading.Lock()


def get_context(device: int = 0, role: str = "") -> Context:
    """Process-wide context per device (created on first use).  ``role``: a second context of the same device with its own
    stream, lock and scratch (the batch hasher keeps its pinned staging route on one, so that decoder processes are served
    while a long GPU decode call holds the main context)."""
    key = device if not role else (device, role)
    with _default_lock:
        ctx = _default.get(key)
        if ctx is None:
            ctx = _default[key] = Context(device)
        return ctx


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library (rank 0 calls it and hands the 128 bytes to the other ranks)."""
    lib = load_library()
    buf = (C.c_uint8 * 128)()
    rc = lib.ke_comm_unique_id(buf)
    if rc != KE_OK:
        raise RuntimeError(f"ke_comm_unique_id failed (rc={rc}): {lib.ke_create_error().decode('utf-8', 'replace')}")
    return bytes(buf)


def cluster_labels(edges: np.ndarray, n_nodes: int) -> np.ndarray:
    """Host-only entry point (no device needed): connected-component labels."""
    lib = load_library()
    edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
    labels = np.empty(n_nodes, np.int64)
    rc = lib.ke_cluster_labels(_addr(edges), len(edges), n_nodes, _addr(labels))
    if rc != KE_OK:
        raise ValueError("ke_cluster_labels: edge endpoint outside [0, n_nodes)")
    return labels
