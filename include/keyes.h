/*
 * keyes.h -- C ABI of libkeyes_hip.so, the MI355X (gfx950) replacement for the
 * src/sig + src/dup hot path of kobato-eyes.
 *
 * The reference is pure Python and has no FFI of its own; each entry point below cites the
 * reference code (paths relative to the reference checkout) whose work it takes over, and
 * INTEGRATION.md shows the ctypes stub a maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success or a negative KE_E* code; ke_last_error(ctx)
 *     returns a human-readable message for the last failure on that context;
 *   - no exceptions cross the boundary, no torch types appear in any signature;
 *   - data pointers may be HOST or DEVICE memory (decided with hipPointerGetAttributes); a pageable host buffer is
 *     copied to a device scratch in chunks of up to 1 GB with hipMemcpyAsync and hashed chunk by chunk (the call blocks);
 *     producers that can write their pixels where they are told -- decoders -- use the pinned staging buffers of
 *     ke_stage_* instead, whose copies overlap the kernels of the previous batch;
 *   - all work of a context is ordered on ONE HIP stream (ke_set_stream / ke_get_stream);
 *     calls return after the work has been ENQUEUED when every pointer is device memory,
 *     and after it has COMPLETED when any output pointer is host memory or the function
 *     returns a count (ke_hamming_scan);
 *   - a context is not re-entrant; use one per thread/device.  The library never falls
 *     back to the CPU: without a gfx950 device ke_create fails.
 */
#ifndef KEYES_H
#define KEYES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KE_ABI_VERSION 1

enum {
    KE_OK = 0,
    KE_EINVAL = -1,     /* bad argument */
    KE_ENODEV = -2,     /* no usable HIP device */
    KE_EHIP = -3,       /* a HIP runtime call failed (see ke_last_error) */
    KE_ENOMEM = -4,
    KE_EUNSUPPORTED = -5
};

/* per-image status written by ke_hash_images (reference: a failed image is dropped,
 * src/core/fastsig.py:36-37) */
enum { KE_IMG_OK = 0, KE_IMG_BAD_SHAPE = 1 };

typedef struct ke_ctx ke_ctx;

/* One candidate edge of the Hamming scan.  a < b are POSITIONS in the hash table handed to
 * ke_hamming_scan (the reference keys edges by file id, src/dup/scanner.py:287-290; the host
 * maps positions to ids).  bands: bit k set <=> band k of x_a ^ x_b is zero (and its bucket is
 * under the pair cap), i.e. the pair meets in bucket (k, value) of src/dup/scanner.py:227-233. */
typedef struct {
    int64_t a;
    int64_t b;
    int32_t h;      /* hamming64(x_a, x_b), src/sig/phash.py:60-63 */
    int32_t bands;
} ke_edge;

/* ---- context ------------------------------------------------------------------------- */
int         ke_abi_version(void);
ke_ctx     *ke_create(int device_id);               /* NULL on failure; see ke_create_error() */
const char *ke_create_error(void);
void        ke_destroy(ke_ctx *ctx);
const char *ke_last_error(ke_ctx *ctx);
int         ke_set_stream(ke_ctx *ctx, void *hip_stream);   /* NULL = the context's own stream */
void       *ke_get_stream(ke_ctx *ctx);
int         ke_synchronize(ke_ctx *ctx);
int         ke_device_info(ke_ctx *ctx, char *name, size_t name_len, int32_t *compute_units,
                           int64_t *total_mem_bytes);

/* device memory helpers for hosts that do not bring their own allocator */
int ke_malloc(ke_ctx *ctx, size_t bytes, void **dev_ptr_out);
int ke_free(ke_ctx *ctx, void *dev_ptr);
/* page-locked host memory (hipHostMalloc): compressed files packed here cross PCIe at link speed and asynchronously, from
 * pageable memory the runtime stages them through its own bounce buffer first.  ke_host_free waits for the context's stream. */
int ke_host_alloc(ke_ctx *ctx, size_t bytes, void **host_ptr_out);
int ke_host_free(ke_ctx *ctx, void *host_ptr);
/* n separate host buffers (srcs[i], sizes[i] bytes) copied to dst + offsets[i] on the host's threads: how a list of files read
 * one by one becomes the single `files` range the decoders take, without an interpreter-level loop over the files. */
int ke_host_pack(uint8_t *dst, const uint8_t *const *srcs, const uint64_t *offsets, const uint64_t *sizes, int64_t n);
/* The files at paths[0..n) read back to back into dst (capacity bytes, normally page-locked) on the host's threads: what
 * `Image.open(path)` of the reference's worker (src/core/fastsig.py:31) does for the bytes, for a whole batch at once.
 * offsets[i] / sizes[i] locate file i; a file that cannot be read has size 0 (the decoders report it as damaged, the caller
 * drops it as the reference drops a file that raises).  *needed_out = bytes the batch needs; when that exceeds capacity nothing
 * is read and KE_ENOMEM comes back, so that the caller can grow the buffer and call again. */
int ke_host_read_files(const char *const *paths, int64_t n, uint8_t *dst, uint64_t capacity, uint64_t *offsets, uint64_t *sizes,
                       uint64_t *needed_out);
int ke_memcpy(ke_ctx *ctx, void *dst, const void *src, size_t bytes);   /* any direction, synchronous */

/* ---- hashing: replaces sig.phash.phash / dhash (src/sig/phash.py:21-57) as driven by
 * core.fastsig._compute_worker (src/core/fastsig.py:24-37) -------------------------------
 * n interleaved 8-bit images.  channels: 1 (mode "L"), 3 (RGB) or 4 (RGBX/RGBA; the fourth
 * byte is ignored, as Pillow's convert("L") ignores it).  Image i starts at
 * pixels + offsets[i] (offsets == NULL: images are packed back to back) and is
 * heights[i] rows of widths[i]*channels bytes, no row padding.  Any byte offset is accepted; the fastest kernels
 * are used for size groups whose images all start on a 4-byte boundary (pad offsets to a multiple of 4 -- the Python
 * host pads to 16 -- when packing a device-resident batch).
 * phash_out / dhash_out: unsigned 64-bit hashes (either may be NULL).  The signed wrap of
 * src/sig/phash.py:29-30 / src/core/fastsig.py:19-21 is the host's reinterpretation.
 * status_out (nullable): KE_IMG_* per image; hashes of failed images are 0.
 *
 * Tuning knob (environment, read at every call): KE_FUSED_MIN_IMAGES = smallest group of equally sized images that is
 * hashed with one workgroup per image; smaller groups are cut into bands of rows so that a few large images still fill
 * the GPU.  Unset: chosen from the image size (about 200 images for 0.4-8 MB images, 512 above).  Results do not depend
 * on it. */
int ke_hash_images(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths,
                   const int32_t *heights, int32_t channels, int64_t n, uint64_t *phash_out,
                   uint64_t *dhash_out, int32_t *status_out);

/* Same, n equally sized images packed back to back (the BASELINE configs). */
int ke_hash_uniform(ke_ctx *ctx, const uint8_t *pixels, int64_t n, int32_t width, int32_t height,
                    int32_t channels, uint64_t *phash_out, uint64_t *dhash_out);

/* The same two calls with one more output: margin_out[i] (float32, host or device, nullable) = min over the 64 DCT
 * coefficients of |coef - mean(AC)| for image i, i.e. the distance of the closest bit decision `coef > mean`
 * (src/sig/phash.py:41-42) from a tie.  pHash bits can only differ between DCT implementations (this library's folded
 * fp64 DCT vs OpenCV's float32 cv2.dct, src/sig/phash.py:38) where this margin is of the order of the implementations'
 * rounding differences (~1e-4 and below); callers count such images to know their exposure.  Needs phash_out. */
int ke_hash_uniform_ex(ke_ctx *ctx, const uint8_t *pixels, int64_t n, int32_t width, int32_t height,
                       int32_t channels, uint64_t *phash_out, uint64_t *dhash_out, float *margin_out);
int ke_hash_images_ex(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths,
                      const int32_t *heights, int32_t channels, int64_t n, uint64_t *phash_out,
                      uint64_t *dhash_out, int32_t *status_out, float *margin_out);

/* ---- turned pHashes: the pHash of all eight orientations of an image, from its one 32x32 tile.  A capability of this
 * library only: the reference has no such feature and no reference line is replaced.
 * Orientation k in 0..7 of a 2-D array a (NumPy notation):
 *     t = a.T if k & 4 else a;   if k & 1: t = t[:, ::-1] (mirror, left <-> right);   if k & 2: t = t[::-1] (flip, top <-> bottom)
 * k = 0 identity, 1 mirror, 2 flip, 3 turn by 180 degrees, 4 transpose, 5 quarter turn clockwise, 6 quarter turn
 * counter-clockwise, 7 transverse; 5 and 6 are each other's inverse, every other k is its own.
 * Turned pHash k of an image is the reference's pHash arithmetic (src/sig/phash.py:38-45: DCT, the 8x8 corner, the float32
 * mean of flat[1:], the bits) applied to orientation k of the image's 32x32 LANCZOS luma tile -- the tile
 * ke_luma_tiles_uniform returns.  Column 0 is the image's pHash, bit for bit.  Columns 1..3 equal the pHash of the really
 * turned image on the images measured (the resize passes commute with a flip); for k >= 4 the two resize passes swap
 * order in the turned file, and its pHash lay at most 2 bits away.
 *
 * ke_tiles_turned       : tile32 = n tiles of 1024 bytes (host or device); turned_out = n * 8 hashes (host or device),
 *                         turned_out[i * 8 + k].
 * ke_hash_images_turned : the arguments of ke_hash_images with turned_out (n * 8, host or device) in place of the two
 *                         hash outputs; grouped and dispatched by the same code, the tiles made by the same kernels.
 *                         A failed image (status_out[i] != 0) has eight zeros. */
int ke_tiles_turned(ke_ctx *ctx, const uint8_t *tile32, int64_t n, uint64_t *turned_out);
int ke_hash_images_turned(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths,
                          const int32_t *heights, int32_t channels, int64_t n, uint64_t *turned_out, int32_t *status_out);

/* ---- pinned staging: the batch boundary of core.fastsig (src/core/fastsig.py:24-37, 65-99: decode in workers, hash,
 * collect in order) as a two-stage pipeline -- north-star step (1), "decodes batches of images to a pinned staging buffer".
 *
 * ke_stage_create allocates n_buffers (1..4) page-locked host buffers of bytes_per_buffer with device twins, result
 * blocks for up to max_images images per batch, and a copy stream.  Per batch:
 *   ke_stage_acquire      -> the next buffer in rotation (blocks only until THAT buffer's previous batch has finished and
 *                            hands its results to the arrays named at its submit); decoders write pixels into it;
 *   ke_stage_submit_hash  -> image i is heights[i] rows of widths[i]*channels[i] bytes at host_ptr + offsets[i] (channels
 *                            per image: 1, 3 or 4; keep offsets multiples of 4, better 16).  Enqueues the H2D copy on the
 *                            copy stream and the hash kernels behind it on the context's stream, then RETURNS: the copy of
 *                            batch k+1 overlaps the kernels of batch k, the host is free to decode into the other buffer.
 *                            phash_out / dhash_out / margin_out (host, nullable) are written when the slot is waited for or
 *                            re-acquired; status_out (KE_IMG_*) is written immediately;
 *   ke_stage_wait         -> blocks until the slot's results are in the caller's arrays (slot -1: every slot, oldest first).
 * Hashes are those of ke_hash_images on the same pixels. */
int ke_stage_create(ke_ctx *ctx, size_t bytes_per_buffer, int64_t max_images, int32_t n_buffers);
/* The same staging on buffers the caller owns: n_buffers page-aligned regions of bytes_per_buffer bytes (a multiple of 256)
 * -- e.g. POSIX shared memory that decoder processes attach to, which is how a Python host gets past its interpreter lock the
 * way the reference does (a process pool, src/core/fastsig.py:83-85).  The library page-locks them (hipHostRegister) until
 * ke_stage_destroy / the next create; the memory must stay mapped that long. */
int ke_stage_create_shared(ke_ctx *ctx, void *const *buffers, size_t bytes_per_buffer, int64_t max_images, int32_t n_buffers);
int ke_stage_destroy(ke_ctx *ctx);
int ke_stage_acquire(ke_ctx *ctx, int32_t *slot_out, uint8_t **host_ptr_out, size_t *bytes_out);
int ke_stage_submit_hash(ke_ctx *ctx, int32_t slot, const uint64_t *offsets, const int32_t *widths, const int32_t *heights,
                         const int32_t *channels, int64_t n, uint64_t *phash_out, uint64_t *dhash_out, int32_t *status_out,
                         float *margin_out);
int ke_stage_wait(ke_ctx *ctx, int32_t slot);

/* ---- JPEG decode on the GPU: `Image.open(path)` + pixel access of the reference's batch hasher (src/core/fastsig.py:31-34;
 * the decode half of north-star step 1) for Huffman-coded JPEGs with 8-bit samples -- sequential files with one interleaved
 * scan and progressive files (spectral selection + successive approximation, any scan script) -- grayscale ("L") or YCbCr at
 * 4:4:4 / 4:2:2 / 4:2:0 / 4:4:0 ("RGB").  The pixels are libjpeg's as Pillow drives it (islow IDCT, fancy upsampling, jdcolor's
 * fixed-point YCbCr -> RGB), bit for bit; everything else (arithmetic coding, 12-bit, CMYK/YCCK, RGB-coded, other samplings,
 * sequential files in several scans, progressive files whose first AC coefficients are not refined to the last bit -- libjpeg
 * smooths those -- and files with a block whose IDCT leaves 16 bits, which no encoder writes and on which libjpeg's C and SIMD
 * routines differ: csrc/ke_jpeg_core.h, ke_idct_islow) is reported KE_JPEG_UNSUPPORTED per file and stays with Pillow,
 * truncated or damaged entropy data KE_JPEG_CORRUPT (Pillow raises on those).  EXIF orientation is not applied -- nor does Image.open.
 *
 * ke_jpeg_probe  : host only.  files + offsets[i] .. + sizes[i] = file i.  widths/heights/channels (1 or 3)/status per file,
 *                  so that the caller can lay out the pixel buffer.
 * ke_jpeg_decode : files in HOST memory (pageable or the pinned buffer of ke_stage_acquire: the compressed bytes are what
 *                  crosses PCIe), pixels_out in DEVICE memory: image i is written packed at pixels_out + out_offsets[i]
 *                  (heights[i] * widths[i] * channels[i] bytes) when status_out[i] == KE_JPEG_OK and left untouched
 *                  otherwise.  One thread per image decodes the entropy-coded segment, then one thread per 8x8 block runs the
 *                  IDCT and one per 4 pixels upsampling + colour: throughput comes from the batch (thousands of files per
 *                  call).  Blocks until the statuses are back; when it returns an error after the upload has begun the stream
 *                  has been synchronised first, so the caller's host buffers are free again either way. */
enum { KE_JPEG_OK_ = 0, KE_JPEG_UNSUPPORTED_ = 1, KE_JPEG_CORRUPT_ = 2 };   /* = KE_JPEG_OK / _UNSUPPORTED / _CORRUPT of the library */
int ke_jpeg_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                  int32_t *heights, int32_t *channels, int32_t *status_out);
int ke_jpeg_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                   uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);
/* ke_jpeg_decode at a reduced size: file i is decoded at 1 / denoms[i] (1, 2, 4 or 8; anything else: KE_EINVAL) -- the pixels
 * Pillow yields after `im.draft(...)` has set that scale up (libjpeg's scale_num / scale_denom: the reduced transforms of
 * jidctred.c per component, upsampling and colour at the reduced sizes; the reference's loader, src/utils/image_io.py:86-88).
 * Image i is ceil(heights[i] / denoms[i]) rows of ceil(widths[i] / denoms[i]) pixels at pixels_out + out_offsets[i].  A file
 * with a block outside the bound of its transform is KE_JPEG_UNSUPPORTED_ as at full size (csrc/ke_jpeg_core.h).  With every
 * denominator 1 the bytes are ke_jpeg_decode's.  Everything else as ke_jpeg_decode. */
int ke_jpeg_decode_scaled(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                          const int32_t *denoms, uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);
/* Restart intervals on separate lanes, opt-in.  KE_JPEG_SPLIT_RESTARTS=1 (environment, read per call; unset, empty or 0: off,
 * and launches and results are exactly as without this path): in both decode calls above a sequential (SOF0 / SOF1) file
 * with a DRI whose restart intervals can be dealt to two lanes or more is decoded one thread per lane instead of one thread
 * per file -- a lane takes g consecutive intervals, g the smallest number that gives a lane at least
 * KE_JPEG_SPLIT_MIN_MCUS MCUs (environment, default 64; a tuning knob, and the tests' way to several lanes in a tiny file)
 * and the file at most 16 384 lanes.  Eligibility rule, checked on the device: with a marker being a position e in
 * [scan_offset, scan_end - 1) where byte e is 0xFF and byte e + 1 is not 0, the entropy-coded segment must hold exactly one
 * marker per interval boundary (intervals - 1 of them) and the k-th, counted from 0, must be RST(k mod 8).  Every other
 * file -- a wrong number, a missing marker, one too many, 0xFF fill bytes in front of one, progressive files, files
 * without DRI or with a DRI that covers the whole image -- is decoded as before and keeps the verdict it gets there.
 * Statuses and pixels do not depend on the variables (csrc/ke_jpeg_restarts.h has the argument).
 * ke_jpeg_last_split: of the last ke_jpeg_decode / ke_jpeg_decode_scaled call on this context, *files_split = the files that
 * were decoded lane-wise and *lanes = the lanes launched for them (either pointer may be NULL); both 0 when the variable is
 * unset.  KE_EINVAL for a NULL context. */
int ke_jpeg_last_split(ke_ctx *ctx, int64_t *files_split, int64_t *lanes);

/* ---- PNG decode on the GPU: the same step for PNG files, Adam7-interlaced or not: 8-bit grayscale ("L"), RGB and RGBA pixels as
 * they are; palette files (1 / 2 / 4 / 8 bits) and grayscale of 1 / 2 / 4 bits as the luma `convert("L")` makes of them --
 * what the reference's hashes see for such a file (src/sig/phash.py:25) -- with channels = 1.  Lossless, hence the pixels of
 * Image.open by construction (zlib/deflate, the five scanline filters).  One thread per image walks the deflate stream
 * (literals to their place, LZ77 copies recorded), one wave per image then makes the copies and one wave per image undoes the
 * filters and checks the stream's Adler-32; throughput comes from the batch.  Chunk CRCs are verified where Pillow verifies
 * them (every chunk but IDAT).  An interlaced file is seven reduced images one after another in the stream: the same kernels,
 * the unfilter pass run once per reduced image and its pixels scattered to their places.  8-bit gray + alpha files decode to
 * their gray samples, what convert("L") makes of mode "LA".  Of an animated PNG frame 0 is decoded -- the IDAT image, what Image.open
 * shows (acTL once, at most one fcTL in front of IDAT and that one for the whole image; other forms: status 1).  16-bit files decode to the 8-bit pixels Pillow opens them to: the
 * samples' high bytes for RGB / RGBA, RGBA (L, L, L, A) for gray + alpha, and for grayscale (Pillow: mode "I;16") the value
 * clipped to 255 that convert("L") / convert("RGB") make of it.  Rows wider than 16384 pixels (8192 at 16 bits):
 * KE_JPEG_UNSUPPORTED_ (1) per file, damaged ones KE_JPEG_CORRUPT_ (2).  Arguments and conventions as ke_jpeg_probe /
 * ke_jpeg_decode; channels is 1, 3 or 4. */
int ke_png_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                 int32_t *heights, int32_t *channels, int32_t *status_out);
int ke_png_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                  uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);

/* ---- BMP files unpacked on the GPU: the same step for the uncompressed files Pillow's BmpImagePlugin opens with its "raw"
 * decoder (src/dup/scanner.py:16-28 ranks the format among the keepers): 24-bit BGR and 32-bit BGRX as RGB, the 32-bit
 * BITFIELDS layouts the plugin lists (byte permutations; RGBA where one of them is alpha), 8-bit palette files as the luma
 * `convert("L")` makes of them -- what the reference's hashes see (src/sig/phash.py:25) -- with channels = 1.  The header is
 * read as BmpImageFile._bitmap reads it (defaults for the colour count and the data offset, padded bottom-up rows unless the
 * height's top byte is 0xFF); the files go to the device as they are and one kernel writes packed top-down rows.  OS/2
 * headers, RLE, 1 / 4 / 16 bits (ke_bmpx_decode), other masks: KE_JPEG_UNSUPPORTED_ (1) per file; pixel data that ends early:
 * KE_JPEG_CORRUPT_ (2) (Pillow: "image file is truncated").  Arguments and conventions as ke_jpeg_probe / ke_jpeg_decode;
 * channels is 1, 3 or 4.  ke_bmp_caveats reports no flags (the format has no orientation tag; alpha shows as channels = 4). */
int ke_bmp_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                 int32_t *heights, int32_t *channels, int32_t *status_out);
int ke_bmp_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                  uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);
int ke_bmp_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out);

/* ---- RLE, 1 / 4-bit and 16-bit BMP files decoded on the GPU: the same step (src/core/fastsig.py:31-34; src/dup/scanner.py:16-28
 * ranks the format among the keepers) for the BMP files ke_bmp_decode returns as unsupported -- for the RLE files a Python loop in
 * Pillow (BmpImagePlugin.BmpRleDecoder: two read(1) per code), the slowest route a scan can meet.  Taken, with the header read as
 * ke_bmp_decode reads it (the same header sizes, limits and defaults): RLE8 (compression 1 with 8 bits) and RLE4 (compression 2
 * with 4 bits), bottom-up and top-down; uncompressed 1-bit and 4-bit palette files (Pillow's P;1 and P;4: the most significant
 * bit or nibble first) -- all of these as the luma `convert("L")` makes of them, channels = 1, an index beyond the palette black,
 * the indices themselves where the palette is the gray identity (mode L), 0 / 255 for the two-colour 1-bit file whose palette
 * is black then white (mode 1); 16-bit files as RGB, channels = 3: compression 0 and BITFIELDS 0x7C00 / 0x3E0 / 0x1F as 5-5-5,
 * BITFIELDS 0xF800 / 0x7E0 / 0x1F as 5-6-5, a field of n bits expanded as floor(v * 255 / (2^n - 1)).  The RLE stream is read
 * as BmpRleDecoder reads it, state for state (ke_bmpx_core.h lists the rules): a run is cut at the row's end and does not wrap,
 * an absolute run spills into the next row, an RLE4 absolute run of an odd n yields n - 1 pixels, the byte skipped behind an
 * absolute run goes by the position in the file, what lies beyond width x height is dropped.  One thread per file walks the
 * codes and writes records, a second kernel expands the records in parallel; 1 / 4 / 16-bit rows are unpacked by one kernel.
 * KE_JPEG_UNSUPPORTED_ (1), left to Pillow although it opens them: RLE8 with another depth than 8 and RLE4 with another than 4;
 * an uncompressed 1- or 4-bit file whose palette passes Pillow's grayscale test in any other way than the two-colour case above
 * (Pillow then reads the packed bytes as 8-bit or 1-bit samples); an RLE file with the black-then-white palette; and -- Pillow
 * raises or not -- an RLE file of more than 2 GiB, more than 256 colours, a palette that leaves the file, other 16-bit masks, compression 4 / 5, the 12-byte
 * OS/2 header, and everything ke_bmp_decode takes.  KE_JPEG_CORRUPT_ (2), where Pillow raises: a stream that ends (end of
 * bitmap, a missing byte) before width x height pixels ("not enough image data"), known only after the walk, so that
 * ke_bmpx_probe can say 0 where ke_bmpx_decode says 2; uncompressed rows that leave the file ("image file is truncated"; the
 * padding of the last stored row may be missing, as for Pillow).  No file is taken by both ke_bmp_decode and ke_bmpx_decode.
 * Arguments and conventions as ke_jpeg_probe / ke_jpeg_decode.  ke_bmpx_caveats reports no flags.  Tuning knob (environment,
 * read at every call): KE_BMPX_SCRATCH_BYTES replaces the device scratch budget of one sub-batch -- the RLE files' records, 16
 * bytes per two bytes of stream, up to 8 times the streams' bytes (default: half the free device memory, 1-32 GB); results do not depend on it. */
int ke_bmpx_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                  int32_t *heights, int32_t *channels, int32_t *status_out);
int ke_bmpx_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                   uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);
int ke_bmpx_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out);

/* ---- GIF files on the GPU: the same step for the first frame of a GIF file -- what Image.open shows, also of an animation --
 * as the luma `convert("L")` makes of it (src/sig/phash.py:25: what the reference's hashes see), channels = 1: palette index ->
 * luma of the local or global palette entry (no palette or an identity gray ramp: the index).  The container is walked as
 * GifImagePlugin walks it, the LZW stream read as Pillow's GifDecode.c reads it (whole sub-blocks only; over when the last
 * pixel is written); one thread per image walks the codes (a string is a copy from earlier output, recorded), one wave per
 * image makes the copies, a last kernel maps indices to luma and puts interlaced rows in place.  A first frame that does not
 * cover the logical screen, code sizes outside 2..8, an end code or the end of the block list before the last pixel, frames
 * of more than 2^23 pixels: KE_JPEG_UNSUPPORTED_ (1) per file (Pillow decides); data that ends early: KE_JPEG_CORRUPT_ (2).
 * Arguments and conventions as ke_jpeg_probe / ke_jpeg_decode.  For the hashing seams only: the reference's SSIM loader turns a
 * palette file into RGB, not luma.  ke_gif_caveats reports no flags. */
int ke_gif_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                 int32_t *heights, int32_t *channels, int32_t *status_out);
int ke_gif_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                  uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);
int ke_gif_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out);

/* ---- TIFF files unpacked on the GPU: the same step for the uncompressed 8-bit files Pillow's TiffImagePlugin opens with its own
 * "raw" decoder (compressed TIFF is libtiff's there and stays with Pillow): gray (BlackIsZero; WhiteIsZero inverted), RGB, RGB
 * with unassociated alpha (RGBA) or an unspecified fourth sample (dropped), palette files as the luma `convert("L")` makes of
 * them (src/sig/phash.py:25), channels = 1.  The first directory is read as ImageFileDirectory_v2.load reads it (both byte
 * orders), the layout derived as TiffImageFile._setup derives it (strips of RowsPerStrip rows); the files go to the device as
 * they are and one kernel gathers the strips into packed rows.  A whitelist: other compression / planar layout / fill order /
 * bit depths / sample formats, tiles, an orientation other than 1, EXIF / GPS directories or an XMP packet (Pillow applies an
 * orientation found there at load time), a strip count that does not match the rows: KE_JPEG_UNSUPPORTED_ (1) per file; a
 * strip that ends behind the file: KE_JPEG_CORRUPT_ (2).  Arguments and conventions as ke_jpeg_probe / ke_jpeg_decode. */
int ke_tiff_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                  int32_t *heights, int32_t *channels, int32_t *status_out);
int ke_tiff_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                   uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);
int ke_tiff_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out);

/* ---- LZW and PackBits TIFF files decoded on the GPU: the same step (src/core/fastsig.py:31-34; src/dup/scanner.py:16-28 ranks the
 * format among the keepers) for the compressed files Pillow hands to libtiff: baseline 8-bit strip files whose Compression is 5
 * (LZW) or 32773 (PackBits), Predictor absent, 1 or 2 (horizontal differencing), in the photometric layouts of ke_tiff_decode and
 * with the same pixels -- gray (WhiteIsZero inverted), RGB, RGBA (unassociated alpha or no ExtraSamples), an unspecified fourth
 * sample dropped, palette files as the luma `convert("L")` makes of them (src/sig/phash.py:25), channels = 1.  Every strip is a
 * stream of its own: one thread per strip walks the LZW codes (MSB-first, 9 to 12 bits, "early" width change, as libtiff's
 * LZWDecode) or the PackBits headers (literals to their place, strings and runs recorded as copies from earlier output), one
 * wave per strip makes the copies, a last kernel undoes the predictor and maps the samples.  The whitelist is tighter than
 * ke_tiff_decode's, because Pillow's parser decides mode and size but libtiff's directory reader decides what is decoded:
 * entries in strictly ascending tag order (no tag twice) out of a fixed list of tags, layout tags SHORT or LONG with their
 * exact counts, one StripOffsets / StripByteCounts value per strip of RowsPerStrip rows, LZW strips that open with the clear code
 * (old-style LSB-first streams do not).  Deflate, JPEG-in-TIFF, CCITT, tiles, planar layout, 16-bit samples, predictor 3, BigTIFF
 * and everything ke_tiff_decode refuses: KE_JPEG_UNSUPPORTED_ (1) per file; a strip that leaves the file or whose stream fails
 * where libtiff's fails (a code not yet in the table, data that ends before the strip is full): KE_JPEG_CORRUPT_ (2).
 * Uncompressed files are ke_tiff_decode's and are refused here (1).  Arguments and conventions as ke_jpeg_probe /
 * ke_jpeg_decode.  ke_tiffc_caveats reports no flags (files with an orientation are refused). */
int ke_tiffc_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                   int32_t *heights, int32_t *channels, int32_t *status_out);
int ke_tiffc_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                    uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);
int ke_tiffc_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out);

/* ---- deflate-compressed TIFF files decoded on the GPU: the same step (src/core/fastsig.py:31-34; src/dup/scanner.py:16-28 ranks the
 * format among the keepers) for the files whose Compression is 8 ("Adobe deflate") or its old alias 32946 -- what Pillow's
 * "tiff_adobe_deflate" / "tiff_deflate", ImageMagick, GIMP and most scanners' "ZIP" option write --, Predictor absent, 1 or 2, in
 * the layouts of ke_tiffc_decode, under the same directory whitelist and with the same pixels.  Every strip is a zlib stream of
 * its own: one kernel gathers the strips into aligned streams, one thread per strip inflates (the PNG path's inflate; literals
 * to their place, matches recorded), one wave per strip makes the copies and holds the strip's Adler-32 against the stream's,
 * the last kernel is ke_tiffc_decode's.  A strip is held to more than libtiff holds it to: one complete zlib stream that
 * yields exactly the bytes of the strip's rows, with a matching Adler-32; bytes behind the stream are ignored.  So a stream
 * that would yield more than the strip holds and one whose four trailer bytes are cut or missing are KE_JPEG_CORRUPT_ (2)
 * although libtiff, which stops when the strip is full, decodes them; every other status 2 -- a wrong trailer, a stream that
 * yields too little, raw deflate, a gzip wrapper, a preset dictionary, a strip that leaves the file -- is a file Pillow raises
 * on.  LZW, PackBits and uncompressed files are refused here (1), as is everything ke_tiffc_decode refuses.  Arguments and
 * conventions as ke_jpeg_probe / ke_jpeg_decode.  ke_tiffz_caveats reports no flags (files with an orientation are refused).
 * Tuning knob (environment, read at every call): KE_TIFFZ_SCRATCH_BYTES replaces the device scratch budget of one sub-batch
 * (default: half the free device memory, 1-32 GB); results do not depend on it. */
int ke_tiffz_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                   int32_t *heights, int32_t *channels, int32_t *status_out);
int ke_tiffz_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                    uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);
int ke_tiffz_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out);

/* ---- lossy WebP files decoded on the GPU: the same step (src/core/fastsig.py:31-34, src/utils/image_io.py:60-138) for WebP files
 * of one VP8 key frame -- the simple format (RIFF / WEBP / "VP8 ") and VP8X files without alpha or animation, their ICCP / EXIF /
 * "XMP " chunks skipped (Pillow applies none of them when it opens the file).  The pixels are libwebp's as Pillow drives it
 * (WebPAnimDecoder, default options): RFC 6386 reconstruction and loop filter, "fancy" chroma upsampling and the 14-bit
 * VP8YUVToR/G/B, bit for bit; channels = 3.  The container and the frame header are read on the host's threads; one thread per
 * image walks the mode and token partitions, one wave per image reconstructs and filters the macroblocks in wavefront order,
 * one thread per pixel upsamples and converts.  Lossless (VP8L), ALPH, ANIM / ANMF, unknown chunks, a VP8X canvas that differs
 * from the frame, an inter frame, show_frame 0, a profile above 3, frames of more than 65 536 macroblocks (16.7 Mpx; the
 * scratch is about 1.2 KB per macroblock) and blocks whose dequantised coefficients leave [-2048, 2048]: KE_JPEG_UNSUPPORTED_ (1)
 * per file; a partition that runs past its end, RIFF or chunk sizes that do not fit the file: KE_JPEG_CORRUPT_ (2).  Arguments
 * and conventions as ke_jpeg_probe / ke_jpeg_decode; ke_webp_probe reads the container and the frame tag only, so a file it
 * reports as taken can still come back refused from ke_webp_decode (whose statuses are final).  ke_webp_caveats sets
 * KE_CAVEAT_ORIENTATION for every file that carries an EXIF or an XMP chunk -- Pillow's getexif() takes an orientation from
 * either -- without reading it: the loader decides.  Tuning knob (environment, read at every call): KE_WEBP_SCRATCH_BYTES caps
 * the device scratch of one sub-batch (default: half the free device memory, 2-160 GB); results do not depend on it. */
int ke_webp_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                  int32_t *heights, int32_t *channels, int32_t *status_out);
int ke_webp_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                   uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);
int ke_webp_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out);

/* ---- lossless WebP files decoded on the GPU: the same step (src/core/fastsig.py:31-34, src/utils/image_io.py:60-138) for WebP
 * files of one VP8L bitstream, which the reference ranks second among its keepers (src/dup/scanner.py:19) -- the simple format
 * (RIFF / WEBP / "VP8L") and VP8X files without animation, their ICCP / EXIF / "XMP " chunks skipped.  The pixels are libwebp's
 * as Pillow yields them, bit for bit: channels = 4 (RGBA) where Pillow opens the file as RGBA -- the VP8L header's alpha bit,
 * whatever a VP8X chunk's alpha flag says --, 3 (RGB, the decoded alpha dropped) otherwise.  The container
 * and the 5-byte header are read on the host's threads; one thread per image walks the stream (prefix codes, colour cache,
 * LZ77), one workgroup per image undoes the transforms (the predictor as a skewed wavefront over rows), one thread per pixel
 * writes the bytes.  Refused per file with KE_JPEG_UNSUPPORTED_ (1): "VP8 " (ke_webp_decode's), ALPH, ANIM / ANMF, unknown
 * chunks, a canvas that differs from the image, a version other than 0, images of more than 16 777 216 pixels (the lossy
 * decoder's cap: the scratch is about 9.2 bytes per pixel plus 96 KiB, 154 MB at the cap) and streams whose prefix codes need
 * more than 64 KiB + 4 bytes per pixel; with KE_JPEG_CORRUPT_ (2): RIFF or chunk sizes that do not fit the file, a stream that
 * ends early, an incomplete or over-subscribed prefix code, a distance that reaches before the first pixel, a transform given
 * twice.  Arguments and conventions as ke_webp_probe / ke_webp_decode; ke_webpl_probe reads the container and the header only,
 * ke_webpl_decode's statuses are final.  ke_webpl_caveats sets KE_CAVEAT_ORIENTATION for an EXIF or XMP chunk (unread: the
 * loader decides) and KE_CAVEAT_TRANSPARENCY for a file of four channels.  KE_WEBP_SCRATCH_BYTES caps the device scratch of
 * one sub-batch here too; results do not depend on it. */
int ke_webpl_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                   int32_t *heights, int32_t *channels, int32_t *status_out);
int ke_webpl_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                    uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);
int ke_webpl_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out);

/* ---- lossy WebP files with an alpha plane decoded on the GPU: the same step (src/core/fastsig.py:31-34, src/utils/image_io.py:60-138)
 * for what `cwebp` and `Image.save("x.webp")` write for a picture with transparency, among the WebP files the reference ranks
 * with its keepers (src/dup/scanner.py:16-28): VP8X files without animation whose alpha flag is set and whose image is one "VP8 "
 * key frame ke_webp_decode would take, with one ALPH chunk directly in front of the frame -- method 0 (the plane's bytes) or 1 (a
 * VP8L stream without its header, the plane in its green channel), any of the four filters, pre-processing 0 or 1 -- or with no
 * ALPH chunk at all (alpha 255); ICCP / EXIF / "XMP " chunks skipped.  The pixels are libwebp's as Pillow yields them
 * (WebPAnimDecoder, non-premultiplied RGBA), bit for bit: channels = 4, the RGB that of the same frame without the plane.  The
 * container, the frame header and the ALPH header byte are read on the host's threads; the frame goes through ke_webp_decode's
 * token and reconstruction kernels, one thread per plane walks a method-1 stream, one workgroup per plane undoes its transforms
 * and the plane's filter (horizontal / vertical: prefix sums mod 256; gradient: a wavefront over anti-diagonals), one thread per
 * pixel converts and writes four bytes.  Refused per file with KE_JPEG_UNSUPPORTED_ (1): files without the alpha flag
 * (ke_webp_decode's, an ALPH chunk without the flag included: Pillow's alpha is not the chunk's then), "VP8L" images
 * (ke_webpl_decode's), ANIM / ANMF, unknown chunks, a chunk between the plane and the frame, everything ke_webp_decode refuses
 * for the frame (its cap of 65 536 macroblocks included) and plane streams whose prefix codes need more than 64 KiB + 4 bytes
 * per pixel; with KE_JPEG_CORRUPT_ (2), as Pillow fails them: two ALPH chunks, an ALPH chunk behind the frame, a chunk of fewer
 * than two bytes, a raw plane shorter than width x height (more bytes are ignored), method 2 / 3, pre-processing 2 / 3, a
 * reserved bit, a plane stream that ends early or is malformed as ke_webpl_decode has it, and what ke_webp_decode calls corrupt.
 * Arguments and conventions as ke_webpl_probe / ke_webpl_decode; ke_webpa_probe reads the container, the frame tag and the ALPH
 * header byte only, ke_webpa_decode's statuses are final.  ke_webpa_caveats sets KE_CAVEAT_ORIENTATION for an EXIF or XMP chunk
 * (unread: the loader decides) and KE_CAVEAT_TRANSPARENCY for every file it takes.  Scratch: about 1.2 KB per macroblock, plus
 * 9.2 bytes per pixel and 96 KiB for a method-1 plane or one byte per pixel for a raw one; KE_WEBP_SCRATCH_BYTES caps the device
 * scratch of one sub-batch here too; results do not depend on it. */
int ke_webpa_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                   int32_t *heights, int32_t *channels, int32_t *status_out);
int ke_webpa_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                    uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);
int ke_webpa_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out);

/* The first frame of animated WebP files (VP8X with the animation flag, ANIM, ANMF chunks) decoded on the GPU -- replaces
 * `Image.open(path)` + pixel access of the reference's batch hasher (src/core/fastsig.py:31-34), which for an animation yields
 * frame 0, for the last class of the WebP files the reference ranks with its keepers (src/dup/scanner.py:16-28) that stayed with
 * Pillow.  The pixels are Pillow's, bit for bit: an all-zero canvas of the VP8X size, channels = 4 where the VP8X alpha flag is
 * set and 3 otherwise whatever the frame carries, the frame's rectangle holding what ke_webp_decode / ke_webpa_decode /
 * ke_webpl_decode give for the same sub-chunks as a still file (unpremultiplied; alpha 255 for a lossy frame without a plane;
 * alpha dropped on an RGB canvas).  Frame 0 is a key frame: its blend and dispose bits and the ANIM background colour change
 * nothing.  The whole container is walked with the demuxer's rules on the host's threads, since Pillow opens an animation only
 * if all of it demuxes; frame 0 runs through the still decoders' kernels as they are, and one workgroup per (image, tile of
 * rows) writes the canvas.  A batch may mix the three codecs.  Refused per file with KE_JPEG_UNSUPPORTED_ (1): files without
 * the animation flag (the still decoders'), a canvas over 2^24 pixels, an odd RIFF size, a VP8X chunk of another size than 10,
 * an ANMF header whose size is not its bitstream's, an ANMF chunk without an image, fewer than 8 stray bytes at the end, and
 * whatever the still decoders refuse for the frame; with KE_JPEG_CORRUPT_ (2), as Pillow fails them: a file cut anywhere inside
 * the RIFF size, reserved VP8X flag bits, the flag without a frame, ALPH / "VP8 " / VP8L / VP8X chunks outside an ANMF chunk,
 * ANMF before ANIM, an ANIM chunk under 6 or an ANMF chunk under 16 bytes, a frame outside the canvas, sub-chunks that run past
 * their ANMF chunk, an ALPH chunk behind its frame or beside a VP8L image, an image in any frame whose first bytes the demuxer
 * fails, and what the still decoders call corrupt in frame 0.
 * Arguments and conventions as ke_webpa_probe / ke_webpa_decode; ke_webpn_probe reports the canvas, reads the container and
 * frame 0's tag, ALPH header byte or stream header only, ke_webpn_decode's statuses are final (the frame's where that fails,
 * else the plane's).  ke_webpn_caveats sets KE_CAVEAT_ORIENTATION for an EXIF or XMP chunk (unread: the loader decides) and
 * KE_CAVEAT_TRANSPARENCY where channels = 4.  The upload is the span of the taken files, later frames included.  Scratch per
 * frame as the still decoder of its codec; the canvas needs none; KE_WEBP_SCRATCH_BYTES caps the device scratch of one
 * sub-batch here too; results do not depend on it. */
int ke_webpn_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                   int32_t *heights, int32_t *channels, int32_t *status_out);
int ke_webpn_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                    uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out);
int ke_webpn_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out);

/* What `Image.open` alone does not tell about a file but the reference's defensive loader acts on (src/utils/image_io.py:60-138:
 * EXIF orientation applied, alpha composited over white): per file a set of KE_CAVEAT_* bits, so that a caller who wants that
 * loader's pixels sends flagged files through it and only the rest through ke_jpeg_decode / ke_png_decode.  ORIENTATION: the
 * file carries an EXIF orientation of 2..8 (JPEG APP1; PNG eXIf or a "Raw profile type ..." text chunk -- or EXIF data that
 * cannot be followed); TRANSPARENCY: a PNG tRNS chunk.  Host only. */
enum { KE_CAVEAT_ORIENTATION = 1, KE_CAVEAT_TRANSPARENCY = 2 };
/* ke_jpeg_caveats also reports the orientation itself in bits 8..11 (1..8) when the tag could be followed: (flags >> 8) & 15. */
int ke_jpeg_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out);
int ke_png_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out);

/* The loader's normalisation itself, for pixels that are on the device already (decoded by ke_jpeg_decode / ke_png_decode):
 * image k (widths[k] x heights[k], channels[k] = 3 or 4, at src + src_offsets[k]) -> RGB at dst + dst_offsets[k], turned as
 * ImageOps.exif_transpose turns it for orientations[k] in 1..8 (src/utils/image_io.py:116-120, src/ui/dup_refine_parallel.py:67-70;
 * 5..8 swap width and height) and, for 4 channels, composited over white as Image.alpha_composite + convert("RGB") do
 * (src/utils/image_io.py:137-151) -- Pillow's integer arithmetic, bit for bit.  src, dst: device; the arrays: host.  Blocks. */
int ke_normalise_rgb(ke_ctx *ctx, const uint8_t *src, const uint64_t *src_offsets, const int32_t *widths, const int32_t *heights,
                     const int32_t *channels, const int32_t *orientations, int64_t n, uint8_t *dst, const uint64_t *dst_offsets);

/* The loader's shrink for an image with a side over 4096 (src/utils/image_io.py:122-124: img.thumbnail((4096, 4096), LANCZOS)),
 * likewise on the device: RGB (width x height at src) -> RGB (out_w x out_h at dst), each band through the resampler that serves
 * the hashes (Pillow's two-pass integer resample, bit-exact); filter as ke_resize_luma_uniform.  The caller computes
 * (out_w, out_h) as Image.thumbnail does (aspect preserved).  src and dst are device memory. */
int ke_thumbnail_rgb(ke_ctx *ctx, const uint8_t *src, int32_t width, int32_t height, int32_t out_w, int32_t out_h, int32_t filter,
                     uint8_t *dst);

/* What Image.thumbnail does to an image more than four times its target (reducing_gap = 2.0; PIL/Image.py resize), on the
 * device: first ke_reduce_rgb -- Image.reduce((fx, fy)) for packed RGB, bit for bit: width x height at src -> ceil(width / fx)
 * x ceil(height / fy) at dst, every pixel the mean of its fx x fy cell in Pillow's fixed point, the partial cells of the last
 * column and row averaged over the pixels they have; fx, fy in 1..255, each on its own -- then ke_thumbnail_rgb_box:
 * ke_thumbnail_rgb through the source rectangle box = {x0, y0, x1, y1} (Pillow's resize box, fractional: (0, 0, w / fx, h / fy)
 * of the reduced image; inside the image or KE_EINVAL).  src and dst are device memory, box is a host array.  Both block. */
int ke_reduce_rgb(ke_ctx *ctx, const uint8_t *src, int32_t width, int32_t height, int32_t fx, int32_t fy, uint8_t *dst);
int ke_thumbnail_rgb_box(ke_ctx *ctx, const uint8_t *src, int32_t width, int32_t height, int32_t out_w, int32_t out_h, int32_t filter,
                         const float *box, uint8_t *dst);

/* Debug/parity hook: the resampled luma tiles the hashes are computed from
 * (reference sig.phash._to_grayscale, src/sig/phash.py:21-26).  tile32_out: n*1024 bytes
 * ([y][x]); tile98_out: n*72 bytes (8 rows x 9 columns); either may be NULL. */
int ke_luma_tiles_uniform(ke_ctx *ctx, const uint8_t *pixels, int64_t n, int32_t width, int32_t height,
                          int32_t channels, uint8_t *tile32_out, uint8_t *tile98_out);

/* ---- candidate scan: replaces the bucket + pair loop of DuplicateScanner.build_clusters
 * (src/dup/scanner.py:227-299) with an all-pairs tiled popcount scan whose predicate is the
 * closed form of that loop:
 *   edge(i,j), i<j  <=>  ids[i] != ids[j]  and  popcount(x_i ^ x_j) <= threshold
 *                        and some band k < band_count has ((x_i ^ x_j) >> k*band_bits) & mask == 0
 *                            (and, with bucket_pair_cap > 0, that bucket holds <= cap pairs)
 *                        and size_ok(sizes[i], sizes[j], size_ratio)   (src/dup/scanner.py:358-370)
 * ids / sizes may be NULL (ids default to positions; no size filter).  size_ratio <= 0 = off.
 * The pair space is dealt tile-by-tile to `part_count` shards; this call evaluates shard
 * `part_index` (one shard per GPU; 0/1 = everything).
 * edges_out: capacity entries (host or device); *n_edges_out = edges found, which may exceed
 * capacity -- the caller then retries with a larger buffer.  Edge order is unspecified.
 * counters_out (nullable, 4 x u64, host): [0] pairs i < j this shard stands for (counted by the tile kernel, one atomic per
 * tile -- the bucket path adds the host's closed form once on the device -- and checked against that closed form: the call
 * fails if they differ; on the bucket path this is the tile partition's count, not the pairs whose edges this shard reports
 * (there a pair (a, b) is reported by shard (a + b) mod part_count): only the sum over all shards, n (n - 1) / 2, has a meaning),
 * [1] sum over emitted edges of the number of shared bands (the reference's "ham=" funnel
 * counter, src/dup/scanner.py:292-299), [2] edges emitted, [3] bucket pairs of the WHOLE table (the same on every
 * shard): sum over bands and band values of C(bucket size, 2) for the buckets the reference walks (size >= 2, under
 * the pair cap) -- its "pairs total=" counter before pairs of equal file id are taken out (src/dup/scanner.py:258-270;
 * the host subtracts those, they need the ids grouped).  With no size filter "size=" equals it. */
int ke_hamming_scan(ke_ctx *ctx, const uint64_t *hashes, const int64_t *ids, const int64_t *sizes, int64_t n,
                    int32_t part_index, int32_t part_count, int32_t threshold, int32_t band_bits,
                    int32_t band_count, double size_ratio, int64_t bucket_pair_cap, ke_edge *edges_out,
                    int64_t capacity, int64_t *n_edges_out, uint64_t *counters_out);

/* The same scan over the pairs that touch newly added entries.  The table is [library | added]: positions
 * first_new .. n-1 are new.  The edge set is exactly { e of ke_hamming_scan(same arguments) : e.b >= first_new } (edges
 * have a < b, so b is the pair's later position), each edge with the h and bands it has there: the pairs between two
 * library entries, which an earlier scan of the library judged, are not visited -- about (n - first_new) * n pairs
 * instead of n^2 / 2, through a trapezoid of the same tiles or the same buckets (KE_SCAN_MODE applies).
 * What depends on the whole table stays whole-table: the bucket sizes bucket_pair_cap is held against (a cap can
 * therefore drop an edge that the library's own scan had, buckets grow with the table) and counters_out[3].
 * counters_out: [0] pairs i < j with j >= first_new this shard stands for, counted and checked as above; over all
 * shards n (n - 1) / 2 - f (f - 1) / 2 with f = first_new.  [1], [2] over the emitted edges.  [3] as above.
 * first_new = 0 is ke_hamming_scan; first_new = n gives no edge and counters_out[0] = 0; outside [0, n] is KE_EINVAL.
 * part_index / part_count, capacity and *n_edges_out behave as above. */
int ke_hamming_scan_from(ke_ctx *ctx, const uint64_t *hashes, const int64_t *ids, const int64_t *sizes, int64_t n,
                         int64_t first_new, int32_t part_index, int32_t part_count, int32_t threshold, int32_t band_bits,
                         int32_t band_count, double size_ratio, int64_t bucket_pair_cap, ke_edge *edges_out,
                         int64_t capacity, int64_t *n_edges_out, uint64_t *counters_out);

/* The same scan between a library and a table of queries, without comparing the queries with each other.  The table is
 * [library | queries]: positions first_new .. n-1 are queries.  The edge set is exactly
 * { e of ke_hamming_scan(same arguments) : e.a < first_new <= e.b }, each edge with the h and bands it has there --
 * first_new * (n - first_new) pairs through a rectangle of the same tiles or the same buckets (KE_SCAN_MODE applies; auto
 * uses the rule of ke_hamming_scan_from against the rectangle's pairs).  The reference has no such scan: this call
 * replaces no reference line, it serves ke_hash_images_turned's eight hashes per file.
 * What depends on the whole table stays whole-table: the bucket sizes bucket_pair_cap is held against and counters_out[3].
 * counters_out: [0] pairs i < first_new <= j this shard stands for, counted per tile and checked against the host's closed
 * form as above; over all shards first_new * (n - first_new).  [1], [2] over the emitted edges.  [3] as above.
 * first_new = 0 or n gives no edge and counters_out[0] = 0; outside [0, n] is KE_EINVAL.  KE_EUNSUPPORTED where the tile
 * kernel is the only path (KE_SCAN_MODE=tiles, bands wider than the bucket tables) and this shard's part of the rectangle
 * has more than 8 388 607 tiles of 1024 x 1024, which one launch does not hold.
 * part_index / part_count, capacity and *n_edges_out behave as above. */
int ke_hamming_scan_cross(ke_ctx *ctx, const uint64_t *hashes, const int64_t *ids, const int64_t *sizes, int64_t n,
                          int64_t first_new, int32_t part_index, int32_t part_count, int32_t threshold, int32_t band_bits,
                          int32_t band_count, double size_ratio, int64_t bucket_pair_cap, ke_edge *edges_out,
                          int64_t capacity, int64_t *n_edges_out, uint64_t *counters_out);

/* The exact scan: every pair of a region within the threshold, with no band predicate.  The edge set is
 *   { (a < b) in the region : popcount(x_a ^ x_b) <= threshold, ids[a] != ids[b], size_ok as ke_hamming_scan }
 * region 0: all pairs, first_new must be 0; region 1: b >= first_new (ke_hamming_scan_from's pairs); region 2:
 * a < first_new <= b (ke_hamming_scan_cross's pairs).  e.h as in the banded scans.  e.bands is the mask ke_hamming_scan gives
 * without a pair cap, computed from band_bits / band_count, and 0 for a pair that shares no band: { e : e.bands != 0 } is
 * exactly the banded call's edge set for the same region and arguments.  There is no bucket_pair_cap: the cap is a property
 * of buckets.
 * The call goes straight to the all-pairs tile kernel: no band histogram, no sorted copy, no bucket statistics;
 * KE_SCAN_MODE is ignored and ke_last_scan_path reports 0.  A shard's tiles are launched in consecutive slices of at most
 * KE_SCAN_TILES_PER_LAUNCH tiles (read once per process; default and ceiling 8 388 607, what one launch holds), so the
 * tile limits of the three calls above do not apply here.
 * counters_out: [0] the region's pairs this shard stands for, counted and checked as above; [1] sum over the edges of the
 * number of shared bands; [2] edges; [3] 0.
 * 0 <= threshold <= 64.  At 64 every pair is within the threshold, every 16-column block of every tile takes the kernel's rare
 * path and every pair goes through the edge cursor: correct, and slow -- the kernel is built for thresholds at which edges are
 * rare.  first_new outside [0, n], a region outside 0..2 and region 0 with first_new != 0 are KE_EINVAL; the other KE_EINVAL
 * cases, part_index / part_count, host or device pointers, capacity and *n_edges_out behave as above. */
int ke_hamming_scan_exact(ke_ctx *ctx, const uint64_t *hashes, const int64_t *ids, const int64_t *sizes, int64_t n,
                          int64_t first_new, int32_t region, int32_t part_index, int32_t part_count, int32_t threshold,
                          int32_t band_bits, int32_t band_count, double size_ratio, ke_edge *edges_out, int64_t capacity,
                          int64_t *n_edges_out, uint64_t *counters_out);

/* ---- ranked search.  A capability of this library only (the reference has no such call): the k nearest entries of a table
 * for each of m queries, by Hamming distance alone.  For query q
 *   S_q = { i < n : popcount(hashes[i] ^ queries[q]) <= max_distance,
 *                   and not (ids && query_ids && ids[i] == query_ids[q]) }
 * and row q of the output is the first min(k, |S_q|) elements of S_q ordered by (distance ascending, position ascending):
 * fully deterministic, ties included.  There is no band predicate, no size filter and no bucket cap -- a pair 4..8 bits apart
 * with a differing bit in every 16-bit band, which ke_hamming_scan never sees, is found here.
 *   index_out    m * k : the positions i, -1 beyond count_out[q]
 *   distance_out m * k : their distances, -1 beyond count_out[q]
 *   count_out    m     : min(k, |S_q|)
 *   within_out   m     : |S_q|                                         (nullable)
 *   histogram_out m * 65 : entries of S_q at each distance 0..64, so 0 above max_distance   (nullable)
 * ids / query_ids may be NULL; with either one NULL nothing is excluded.  1 <= k <= KE_NEAREST_MAX_K, 0 <= max_distance <= 64,
 * n, m >= 0, n <= 2^31 - 1; anything else is KE_EINVAL.  n == 0: every count 0, the rows -1.  m == 0: KE_OK, nothing touched.
 * Every pointer may be host or device memory, each on its own.  Exhaustive: n * m pairs, the table read twice per query by
 * one workgroup.  Blocks.  ke_last_kernel_ms kind 9 times the kernel. */
#define KE_NEAREST_MAX_K 1024
int ke_hamming_nearest(ke_ctx *ctx, const uint64_t *hashes, const int64_t *ids, int64_t n, const uint64_t *queries,
                       const int64_t *query_ids, int64_t m, int32_t k, int32_t max_distance, int64_t *index_out,
                       int32_t *distance_out, int32_t *count_out, int64_t *within_out, uint32_t *histogram_out);

/* The reference's "size=" funnel counter (src/dup/scanner.py:268-270 with _passes_size_ratio, :358-370): over every band
 * and band value whose bucket the reference walks (>= 2 members, under the pair cap), the member pairs that pass the size
 * filter -- pairs of equal file id included (the host takes those out, as for counters_out[3] of ke_hamming_scan).  A log
 * figure, not part of the candidate set: asked for separately so that a scan nobody watches does not pay for it.
 * size_ratio must be > 0.  hashes / sizes: host or device.  Blocks. */
int ke_band_pairs_after_size(ke_ctx *ctx, const uint64_t *hashes, const int64_t *sizes, int64_t n, int32_t band_bits,
                             int32_t band_count, double size_ratio, int64_t bucket_pair_cap, uint64_t *count_out);

/* Connected components of the candidate graph (DisjointSet, src/dup/scanner.py:176-200,
 * 304-318; ClusterBuilder union-find, src/dup/cluster.py:30-46).  HOST function, no device
 * work: label_out[v] = smallest node of v's component for v < n_nodes. */
int ke_cluster_labels(const ke_edge *edges, int64_t n_edges, int64_t n_nodes, int64_t *label_out);

/* ---- multi-GPU exchange on RCCL (xGMI): one process per GPU, image i on rank i mod world.  The reference has no
 * counterpart (it is a single process, src/core/fastsig.py:81-85 is its only parallelism); these are the two exchange
 * steps of the sharded path: the hash table before the scan, the edge lists after it.  RCCL (librccl.so.1) is bound at
 * first use; a process that already carries one -- PyTorch's -- is joined.  `comm` is an ncclComm_t as void*: made by
 * ke_comm_create from a 128-byte unique id (ke_comm_unique_id on rank 0, distributed by the host), or any communicator
 * of the calling process whose ranks are the ranks of this job.  All of it is ordered on the context's stream.
 *
 * ke_allgather_u64   : plain ncclAllGather, n_local entries per rank, rank order (device pointers).
 * ke_allgather_hashes: every rank passes its ceil(n_total / world) local hashes (image rank + k * world at slot k, padded);
 *                      table[i] = hash of image i for i < n_total on every rank: ONE all-gather + a reorder kernel.
 * ke_allgather_edges : per-rank edge lists of ke_hamming_scan (device, n_local valid records) -> all edges of all ranks in
 *                      a host array, rank by rank; *n_total_out may exceed capacity (then only whole records that fit are
 *                      written; retry larger).  counts_out (nullable, world entries): edges per rank.  ONE all-gather of
 *                      fixed-width records [count | first K edges] and one device-to-host copy; K follows the largest list
 *                      seen on this context, a second gather happens only when a list outgrows it.  Blocks. */
int ke_comm_unique_id(uint8_t *id_out /* 128 bytes */);
int ke_comm_create(ke_ctx *ctx, const uint8_t *unique_id, int32_t world, int32_t rank, void **comm_out);
int ke_comm_destroy(ke_ctx *ctx, void *comm);
int ke_allgather_u64(ke_ctx *ctx, void *comm, int32_t world, const uint64_t *local, int64_t n_local, uint64_t *gathered);
int ke_allgather_hashes(ke_ctx *ctx, void *comm, int32_t world, const uint64_t *local, int64_t n_total, uint64_t *table);
/* the reorder step on its own, for hosts that gather with another library: gathered = world shards of ceil(n_total / world)
 * entries in rank order (device), table[i] = gathered[(i mod world) * per + i / world] */
int ke_interleave_shards(ke_ctx *ctx, const uint64_t *gathered, int32_t world, int64_t n_total, uint64_t *table);
int ke_allgather_edges(ke_ctx *ctx, void *comm, int32_t world, const ke_edge *local, int64_t n_local, ke_edge *merged_out,
                       int64_t capacity, int64_t *n_total_out, int64_t *counts_out);

/* ---- SSIM refine: replaces dup.refine._compute_ssim (src/dup/refine.py:44-52 ->
 * skimage.metrics.structural_similarity, 7x7 uniform window, float32, data_range 1) for
 * pairs of equally sized images.  images: n_images interleaved images of width x height x
 * channels (1, 3 or 4; luma is taken exactly as convert("L") does), packed back to back.
 * pair_a/pair_b index into them.  ssim_out[k] is NaN when width or height < 7. */
/* Two kernels compute it.  KE_SSIM_FAST (default): every 7x7 window sum is an exact integer (luma 0..255) carried in
 * float32, variances formed without cancellation error -- equal to skimage's float32 arithmetic up to what skimage's own
 * intermediates round away (measured |delta| < 1e-5; the bar of BASELINE.json is 1e-4); images of fewer than 4096
 * windows ((w-6)*(h-6)) always take the exact kernel, where a single window's rounding is not averaged out.  KE_SSIM_EXACT: every float32 /
 * float64 rounding of scipy.ndimage.uniform_filter and of skimage's elementwise steps reproduced one by one, bit-identical
 * to the oracle, 3-4x slower. */
enum { KE_SSIM_FAST = 0, KE_SSIM_EXACT = 1 };
int ke_ssim_set_mode(ke_ctx *ctx, int32_t mode);
int ke_ssim_pairs_uniform(ke_ctx *ctx, const uint8_t *images, int64_t n_images, int32_t width,
                          int32_t height, int32_t channels, const int64_t *pair_a, const int64_t *pair_b,
                          int64_t n_pairs, double *ssim_out);

/* The whole of dup.refine._compute_ssim (src/dup/refine.py:44-52) for pairs of images of ANY sizes: per pair the common
 * size (min width, min height) (src/dup/refine.py:45-47), ImageOps.fit(convert("L"), size, BICUBIC) of both
 * (ke_fit_luma_uniform's arithmetic), then the SSIM above.  Image i: heights[i] rows of widths[i]*channels bytes at
 * pixels + offsets[i] (offsets NULL: packed back to back); pixels host or device, everything else host arrays.
 * Work is grouped: one fit launch per (source size, common size), one SSIM launch per common size.
 * ssim_out[k]: the score, NaN where status_out[k] != KE_PAIR_OK.  status_out (nullable): KE_PAIR_OK, KE_PAIR_TOO_SMALL (the
 * common size is under 7 pixels: skimage raises "win_size exceeds image extent"), KE_PAIR_BAD_IMAGE (an index outside
 * [0, n_images) or an image with a non-positive size). */
enum { KE_PAIR_OK = 0, KE_PAIR_TOO_SMALL = 1, KE_PAIR_BAD_IMAGE = 2 };
int ke_ssim_pairs(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths, const int32_t *heights,
                  int32_t channels, int64_t n_images, const int64_t *pair_a, const int64_t *pair_b, int64_t n_pairs,
                  double *ssim_out, int32_t *status_out);

/* A capability of this library only (the reference has no turned duplicates): the luma plane of one of the eight orientations
 * of a picture.  Orientation k in 0..7 as python's turned.ORIENTATIONS: transposed if k & 4, then mirrored (left <-> right) if
 * k & 1, then flipped (top <-> bottom) if k & 2; 0 is a plain luma copy.  Image i (widths[i] x heights[i], channels[i] = 1, 3 or 4,
 * the fourth ignored, at src + src_offsets[i]) -> the convert("L") luma of orientation orientations[i] of it, 1 byte per pixel,
 * rows packed, at dst + dst_offsets[i]: heights[i] x widths[i] for k & 4.  Luma is per pixel, so the plane is byte for byte the
 * luma of the turned picture.  src, dst: device; the arrays: host.  Blocks. */
int ke_turn_luma(ke_ctx *ctx, const uint8_t *src, const uint64_t *src_offsets, const int32_t *widths, const int32_t *heights,
                 const int32_t *channels, const int32_t *orientations, int64_t n, uint8_t *dst, const uint64_t *dst_offsets);

/* ke_ssim_pairs with one more array: pair k is image pair_a[k] against orientation orient_b[k] (0..7, as ke_turn_luma) of
 * image pair_b[k].  The common size is taken from b's turned size (swapped for k & 4); the fit, the SSIM and the statuses are
 * ke_ssim_pairs'.  Every distinct (image, orientation != 0) of a call is turned once, by one ke_turn_luma launch into scratch
 * of 1 byte per pixel, and enters the fit as a one-channel source.  orient_b NULL or all zeros: ke_ssim_pairs' answers, bit for
 * bit.  An orientation outside 0..7: KE_EINVAL, nothing launched. */
int ke_ssim_pairs_turned(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths, const int32_t *heights,
                         int32_t channels, int64_t n_images, const int64_t *pair_a, const int64_t *pair_b, const int32_t *orient_b,
                         int64_t n_pairs, double *ssim_out, int32_t *status_out);

/* ---- bordered copies.  A capability of this library only (the reference has no such feature): the CONTENT BOX of an image
 * and the pHash of the image cut to it, for finding a letterboxed, pillarboxed, framed or white-margined copy of a picture.
 *
 * Image i: heights[i] rows of widths[i] * channels bytes at pixels + offsets[i] (offsets NULL: packed back to back), any byte
 * offset legal; channels 1, 3 or 4, the fourth byte ignored as the hashes ignore it.
 *   ref[c] = pixel (0, 0), channel c.  A pixel DIFFERS when max over c of |p[c] - ref[c]| > tolerance (0..255).
 *   No pixel differs: the image has no box, four zeros.  Otherwise the box is (x0, y0, x1, y1): the smallest x and y of a
 *   differing pixel and the largest plus one -- Pillow's getbbox convention.  In Pillow (RGBA first through convert("RGB")):
 *       bg   = Image.new(im.mode, im.size, im.getpixel((0, 0)))
 *       mask = ImageChops.difference(im, bg).point(lambda v: 255 if v > tol else 0)
 *       box  = mask.getbbox()
 *   A box QUALIFIES for a trimmed hash when it exists, both its sides are >= 8, and it cuts at least 2 % off one axis:
 *   (w - bw) * 50 >= w or (h - bh) * 50 >= h.  (A one-pixel trim would only double the plain hash's edges.)
 *   The TRIMMED pHash of an image with a qualifying box is ke_hash_images' pHash of the box's pixels (im.crop(box)).
 *
 * ke_content_boxes: boxes_out[4 i .. 4 i + 3] = the box of image i, four zeros for an image without one or with a status other
 *   than KE_IMG_OK (status_out nullable).  One pass over the pixels, which are never read outside
 *   [pixels + offsets[i], + w * h * channels).  pixels: host or device; everything else host arrays.
 * ke_crop_pack: rows [y0, y1) x columns [x0, x1) of image i (boxes[4 i ..], inside the image and not empty, else KE_EINVAL) ->
 *   dst + dst_offsets[i], rows packed, (x1 - x0) * channels bytes each; nothing outside those bytes is written.  src, dst:
 *   device; the arrays: host.
 * ke_hash_images_trimmed: the boxes, the qualifying rule on the host, ke_crop_pack of the qualifying images into scratch of at
 *   most 1 GiB a chunk (or one crop, if larger), ke_hash_images on the crops.  has_out[i] = 1 and phash_out[i] = the trimmed
 *   pHash where the box qualifies; otherwise has_out[i] = 0 and phash_out[i] = 0, and boxes_out still holds the box.  A failed
 *   image has status != KE_IMG_OK and zeros.  pixels: host (staged in chunks of at most 1 GiB) or device; the rest host arrays.
 * ke_crop_luma: the same rows and columns of image i (channels[i] = 1, 3 or 4, the fourth byte ignored; any other count, an
 *   empty box or one not inside its image: KE_EINVAL, nothing launched) -> their convert("L") luma (ke_turn_luma's, orientation
 *   0), 1 byte per pixel, rows packed, at dst + dst_offsets[i]; any byte offset is legal on both sides, nothing is read outside
 *   [src + src_offsets[i], + w * h * channels[i]) and nothing written outside the plane.  One streaming pass: no LDS, a wave a
 *   box row, aligned dwords on both sides.  src, dst: device; the arrays: host.
 * All four block.  ke_last_kernel_ms kind 5 times the box kernel, kind 6 the crop kernel (of the last chunk), kind 7 the
 * luma-crop kernel. */
int ke_content_boxes(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths, const int32_t *heights,
                     int32_t channels, int64_t n, int32_t tolerance, int32_t *boxes_out, int32_t *status_out);
int ke_crop_pack(ke_ctx *ctx, const uint8_t *src, const uint64_t *src_offsets, const int32_t *widths, const int32_t *heights,
                 int32_t channels, const int32_t *boxes, int64_t n, uint8_t *dst, const uint64_t *dst_offsets);
int ke_hash_images_trimmed(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths, const int32_t *heights,
                           int32_t channels, int64_t n, int32_t tolerance, uint64_t *phash_out, int32_t *boxes_out, uint8_t *has_out,
                           int32_t *status_out);
int ke_crop_luma(ke_ctx *ctx, const uint8_t *src, const uint64_t *src_offsets, const int32_t *widths, const int32_t *heights,
                 const int32_t *channels, const int32_t *boxes, int64_t n, uint8_t *dst, const uint64_t *dst_offsets);

/* ke_ssim_pairs with two more arrays, for re-checking a bordered copy on its content box: pair k is box box_a[4 k ..] of image
 * pair_a[k] against box box_b[4 k ..] of image pair_b[k], boxes as (x0, y0, x1, y1).  A NULL array, a box of four zeros and the
 * box (0, 0, w, h) mean the image as it lies: that side enters the fit straight from `pixels`, as in ke_ssim_pairs.  Any other
 * box must be non-empty and inside its image, else KE_EINVAL naming the pair, nothing launched.  The common size is the minimum
 * of the two VIEW sizes; the fit, the SSIM and the statuses are ke_ssim_pairs'.  Every distinct (image, box) of a call is cut
 * out once, by one ke_crop_luma launch into scratch of 1 byte per pixel, and enters the fit as a one-channel source of the
 * box's size; fit groups are (view w, view h, cropped or not).
 * CROP, THEN FIT.  The box is not folded into the fit's resample box: Pillow's resampler clips its taps to the image it is given,
 * not to the box, so the margin would bleed into the crop's edge.  As it is, the answer is bit-equal to ke_ssim_pairs on images
 * that hold the crops (a.crop(box_a), b.crop(box_b)): luma is per pixel and the resampler is bit-exact. */
int ke_ssim_pairs_boxed(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths, const int32_t *heights,
                        int32_t channels, int64_t n_images, const int64_t *pair_a, const int64_t *pair_b, const int32_t *box_a,
                        const int32_t *box_b, int64_t n_pairs, double *ssim_out, int32_t *status_out);

/* ---- copies that are bordered AND turned.  A capability of this library only (the reference has neither feature): a VIEW of
 * an image is a box of it, then an orientation of that crop -- turned.turn(k, image[y0:y1, x0:x1]), crop first.
 *
 * ke_crop_turn_luma: image i (widths[i] x heights[i], channels[i] = 1, 3 or 4, the fourth byte ignored, at src + src_offsets[i]),
 *   box boxes[4 i ..] = (x0, y0, x1, y1), orientation orientations[i] (0..7, as ke_turn_luma) -> the convert("L") luma of that
 *   orientation of the box's pixels, 1 byte per pixel, rows packed, at dst + dst_offsets[i]: (x1 - x0) x (y1 - y0), sides swapped
 *   for k & 4; byte for byte the luma of Pillow's crop(box).transpose(...).  A channel count other than 1, 3, 4, an empty box or
 *   one not inside its image, an orientation outside 0..7: KE_EINVAL, nothing launched.  n == 0: KE_OK.  Any byte offset is
 *   legal on both sides; nothing is read outside [src + src_offsets[i], + w * h * channels[i]) -- the margin pixels beside the box
 *   may be -- and nothing is written outside the plane.  ke_turn_luma's kernel shape (64 x 64 destination tiles through LDS
 *   twice, aligned dwords on both sides) with the tile's source rectangle at the box's origin and the image's row pitch.  src,
 *   dst: device; the arrays: host.  Blocks.  ke_last_kernel_ms kind 8 times the kernel.
 * ke_ssim_pairs_viewed: ke_ssim_pairs_boxed with ke_ssim_pairs_turned's orient_b: pair k is box_a of image pair_a[k] against
 *   orientation orient_b[k] of box_b of image pair_b[k].  CROP, THEN TURN, THEN FIT.  The common size is the minimum of the two
 *   view sizes, b's swapped for k & 4; the fit, the SSIM and the statuses are ke_ssim_pairs'.  Every distinct (image, box,
 *   orientation) of a call is made once into scratch of 1 byte per pixel, by one launch per kind of view: a whole picture (box
 *   NULL, zeros or (0, 0, w, h)) at orientation 0 enters the fit straight from `pixels`; a real box at 0 is ke_crop_luma's; a
 *   whole picture turned is ke_turn_luma's; a real box turned is ke_crop_turn_luma's.  orient_b NULL or all zeros:
 *   ke_ssim_pairs_boxed's answers, bit for bit; both box arrays NULL: ke_ssim_pairs_turned's.  A bad box or orientation:
 *   KE_EINVAL naming the pair, nothing launched.
 * ke_hash_images_turned_trimmed: one call for what ke_hash_images_turned and ke_hash_images_trimmed give, and the turned hashes
 *   of the crop.  turned_out[8 i + k]: exactly ke_hash_images_turned's.  boxes_out, has_out: exactly ke_hash_images_trimmed's.
 *   trimmed_turned_out[8 i + k]: turned pHash k of im.crop(box) -- the pHash arithmetic on orientation k of the crop's 32 x 32
 *   tile, so column 0 is the trimmed pHash --, eight zeros where the box does not qualify.  THE BOX IS ALWAYS FOUND ON THE PICTURE
 *   AS IT LIES, with the reference pixel at (0, 0): turning does not commute with that choice of corner, so the box of a turned
 *   picture need not be the turned box.  Built from the existing passes: the box kernel, ke_crop_pack in chunks of at most 1 GiB,
 *   ke_hash_images_turned on the pixels and on the crops.  pixels: device, or host -- then every chunk of at most 1 GiB is
 *   staged once and both passes walk it on the device; the rest host arrays.  Blocks. */
int ke_crop_turn_luma(ke_ctx *ctx, const uint8_t *src, const uint64_t *src_offsets, const int32_t *widths, const int32_t *heights,
                      const int32_t *channels, const int32_t *boxes, const int32_t *orientations, int64_t n, uint8_t *dst,
                      const uint64_t *dst_offsets);
int ke_ssim_pairs_viewed(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths, const int32_t *heights,
                         int32_t channels, int64_t n_images, const int64_t *pair_a, const int64_t *pair_b, const int32_t *box_a,
                         const int32_t *box_b, const int32_t *orient_b, int64_t n_pairs, double *ssim_out, int32_t *status_out);
int ke_hash_images_turned_trimmed(ke_ctx *ctx, const uint8_t *pixels, const uint64_t *offsets, const int32_t *widths,
                                  const int32_t *heights, int32_t channels, int64_t n, int32_t tolerance, uint64_t *turned_out,
                                  uint64_t *trimmed_turned_out, int32_t *boxes_out, uint8_t *has_out, int32_t *status_out);

/* ---- shipped refine stage ("next" row of SURVEY 8f): replaces the per-file work of
 * ui.dup_refine_parallel -- tile_ahash_bits (src/ui/dup_refine_parallel.py:59-83), _load_small_gray
 * (:203-207) and _mae01 (:208-210).
 *
 * ke_resize_luma_uniform: n equally sized images -> n luma thumbnails of out_h rows x out_w bytes, exactly
 * image.convert("L").resize((out_w, out_h), filter) of Pillow; filter 0 = LANCZOS (src/sig/phash.py:24),
 * 1 = BILINEAR (src/ui/dup_refine_parallel.py:70, :204), 2 = BICUBIC (src/dup/refine.py:48).
 * ke_tile_ahash: thumbnails of side grid*tile -> ceil((grid*tile)^2 / 64) little-endian u64 words per image;
 * bit i (order gy, gx, ty, tx) = pixel > mean of its tile.
 * ke_sad_pairs: sum |a - b| over two thumbnails of `pixels` bytes; MAE = sad / pixels / 255 on the host. */
enum { KE_FILTER_LANCZOS = 0, KE_FILTER_BILINEAR = 1, KE_FILTER_BICUBIC = 2 };
int ke_resize_luma_uniform(ke_ctx *ctx, const uint8_t *pixels, int64_t n, int32_t width, int32_t height,
                           int32_t channels, int32_t out_w, int32_t out_h, int32_t filter, uint8_t *tiles_out);
/* ke_fit_luma_uniform: ImageOps.fit(image.convert("L"), (out_w, out_h), filter) of Pillow for n equally sized
 * images -- centre crop to the target aspect ratio (default bleed 0, centering 0.5/0.5; the crop box is formed
 * in Python's float arithmetic and handed to the resampler in single precision, as Pillow does), then
 * Image.resize(size, filter, box=crop).  This is how src/dup/refine.py:44-49 brings two images of different
 * size to the common (min width, min height) before SSIM; filter 2 = BICUBIC is the reference's choice.
 * A target equal to the input size is a plain luma conversion. */
int ke_fit_luma_uniform(ke_ctx *ctx, const uint8_t *pixels, int64_t n, int32_t width, int32_t height,
                        int32_t channels, int32_t out_w, int32_t out_h, int32_t filter, uint8_t *tiles_out);
int ke_tile_ahash(ke_ctx *ctx, const uint8_t *tiles, int64_t n, int32_t grid, int32_t tile, uint64_t *bits_out);
int ke_sad_pairs(ke_ctx *ctx, const uint8_t *thumbs, int64_t n_thumbs, int64_t pixels, const int64_t *pair_a,
                 const int64_t *pair_b, int64_t n_pairs, uint64_t *sad_out);

/* ---- synthetic corpus (BASELINE configs; DESIGN.md "Synthetic data") --------------------
 * Writes images [first_index, first_index+n) of the counter-based corpus as packed RGB into
 * device or host memory; ke_synth_hashes writes the scan-only hash table. */
int ke_synth_rgb(ke_ctx *ctx, uint64_t seed, int64_t first_index, int64_t n, int32_t width, int32_t height,
                 uint8_t *rgb_out);
/* The same generator for an arbitrary list of corpus positions (host or device array): image k of the output is
 * corpus image indices[k].  A rank that has to evaluate a pair whose images live on another rank regenerates them
 * this way (SSIM stage); rgb_out must be device memory. */
int ke_synth_rgb_indexed(ke_ctx *ctx, uint64_t seed, const int64_t *indices, int64_t n, int32_t width, int32_t height,
                         uint8_t *rgb_out);
int ke_synth_hashes(ke_ctx *ctx, uint64_t seed, int64_t n, uint64_t *hashes_out);

/* ---- timing hook for bench.py: wall time of the kernels enqueued by the LAST call of the
 * named kind on this context, measured with hipEvents on the context's stream.
 * kind: 0 = hash kernel(s), 1 = scan kernel, 2 = ssim kernel, 3 = synth kernel, 4 = JPEG / PNG decode kernels,
 * 5 = content-box kernel, 6 = crop kernel, 7 = luma-crop kernel, 8 = crop-and-turn kernel, 9 = nearest-neighbour kernel.
 * Returns milliseconds, or a negative value if nothing was recorded.  Blocks until done. */
double ke_last_kernel_ms(ke_ctx *ctx, int32_t kind);

/* ---- for the tests of the scratch budgets (KE_<KIND>_SCRATCH_BYTES; results do not depend on them, so nothing else shows
 * that one was honoured): the number of sub-batches in which the last decode call on this context that runs the shared
 * sub-batch loop (jpeg, png, bmpx, gif, tiffc, tiffz, webp, webpl, webpa, webpn; bmp and tiff have no scratch and need none) worked
 * off the images it accepted.  0 before any such call; -1 for a NULL context. */
int64_t ke_last_decode_sub_batches(ke_ctx *ctx);

/* ---- for the tests of the scan's two paths (the result does not depend on the path): which one the last ke_hamming_scan
 * on this context with n >= 2 took, as chosen on the device: 0 = all-pairs tiles, 1 = band buckets.  -1 before any such
 * call and for a NULL context.  KE_SCAN_MODE=auto|tiles|buckets (environment, read once per process) forces a path;
 * `buckets` still runs tiles where the bucket path is not built (band tables over 2^18 bins, n >= 2^32, no memory for the
 * sorted copy of the table: 12 bytes per hash and band). */
int32_t ke_last_scan_path(ke_ctx *ctx);

/* ---- for the tests of the general resampler (the pixels do not depend on the plan): what the last group of images that
 * ke_resize_luma_uniform, ke_fit_luma_uniform, ke_ssim_pairs' fit step, ke_thumbnail_rgb or ke_thumbnail_rgb_box resampled on
 * this context was launched as.  A call that works its images off in several groups reports the last one.  The hash calls
 * do not update it: their fallback tiles run the same two resamplers, but not through this entry.
 *   [0] 0 = generic passes (one thread per output, Pillow's two passes), 1 = banded (horizontal taps per row band, vertical
 *       taps from the transposed columns)
 *   [1] chunks each output's horizontal tap window is cut into (1, 2, 4, 8, 16 or 32)
 *   [2] dwords per chunk (8, 16, 24 or 32)
 *   [3] horizontal launches (the outputs are split when their chunks exceed the 256 lanes of a workgroup)
 *   [4] row bands per image
 *   [5] 1 = rows read through the funnel-shift loader (width no multiple of 4), 0 = whole dwords
 *   [6] 1 = vertical taps on the matrix cores, 0 = on the VALU (more than 128 output rows, or KE_VTILE_VALU set)
 *   [7] 1 = vertical pass first (generic only: Pillow's rule for sources over 100 times taller than wide)
 * Entries that do not apply to the path taken are -1 ([1]..[6] for generic, [7] for banded); all are -1 before any such
 * call.  KE_EINVAL for a NULL context or a NULL plan_out. */
int ke_last_resize_plan(ke_ctx *ctx, int32_t plan_out[8]);

/* ---- for the tests of the SSIM kernels (the scores do not depend on the plan beyond the kernel's own bar): what the last SSIM
 * launch on this context -- ke_ssim_pairs_uniform, or the last common size of ke_ssim_pairs and of the turned, boxed and viewed
 * pair calls -- was launched as.  The rules are in csrc/ke_ssim_plan.h.
 *   [0] kernel: 0 = NaN fill (a side under 7), 1 = exact (fp64 carries), 2 = fast (integer sums)
 *   [1] pixels per lane (4 or 8)
 *   [2] 1 = rows read as whole dwords, 0 = through the funnel-shift loader
 *   [3] column blocks per image
 *   [4] interior columns per block (250, 248, 506 or 504)
 *   [5] interior rows per band (exact: 64; fast: 14 .. 126 in steps of 7, by the work in the launch)
 *   [6] row bands per image
 *   [7] why [2] is what it is: 0 = aligned, 1 = the width is no multiple of 4, 2 = the base address or the image size is no
 *       multiple of 4, 3 = blocks of 248 / 504 columns would add a block
 * [1]..[7] are -1 for the NaN fill; all are -1 before any such call.  KE_EINVAL for a NULL context or a NULL plan_out. */
int ke_last_ssim_plan(ke_ctx *ctx, int32_t plan_out[8]);

#ifdef __cplusplus
}
#endif
#endif /* KEYES_H */
