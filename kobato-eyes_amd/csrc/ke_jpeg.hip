// ke_jpeg.hip -- JPEG decoding on the GPU (sequential and progressive Huffman files): the decode step in front of the hash path (north-star step 1; SURVEY 8 f2,
// "GPU-side JPEG decode").  Replaces `Image.open(path)` + pixel access of the reference's batch hasher
// (src/core/fastsig.py:31-34) for the files it can take; the pixels are libjpeg's, bit for bit (ke_jpeg_core.h says which
// of its routines are restated), so the hashes are those of the Pillow route.
//
// Three kernels per batch:
//   ke_jpeg_entropy : ONE THREAD PER IMAGE walks the image's entropy-coded segment (Huffman decoding is sequential within a
//                     scan; the parallelism is across the batch -- a 16 384-image batch is one wave per CU, 100 000 images
//                     fill the chip) and writes every block's coefficients (int16) whole;
//   ke_jpeg_entropy_prog : the same for progressive files, scan after scan into a zeroed coefficient array;
//   ke_jpeg_find_restarts + ke_jpeg_entropy_rst : opt-in (KE_JPEG_SPLIT_RESTARTS), for sequential files with restart intervals:
//                     one thread per group of intervals instead of one per image (ke_jpeg_restarts.h);
//   ke_jpeg_idct    : one thread per 8x8 block: dequantise, jpeg_idct_islow, samples into padded component planes;
//   ke_jpeg_colour  : one thread per 4 output pixels: fancy upsampling + YCbCr -> RGB (or the luma plane as it is), packed
//                     8-bit pixels where ke_hash_images / ke_ssim_pairs expect them.
// Compressed bytes cross PCIe (a tenth of the pixels); files the parser refuses (arithmetic coding, CMYK, ...) are reported per
// image and stay with Pillow.
#include <algorithm>
#include <numeric>

#include <chrono>
#include <memory>
#include <cstdio>

#include "ke_decode_batch.h"
#include "ke_jpeg_parse.h"
#include "ke_jpeg_restarts.h"

namespace {

struct KeJpegDev {                 // per image, device side
    KeJpegInfo info;
    uint64_t file_off;             // into the uploaded file bytes
    uint64_t coef_off;             // int16 units into the coefficient array
    uint64_t plane_off[3];         // bytes into the plane array
    uint64_t out_off;              // bytes into the caller's pixel buffer
    int32_t block_base[3];         // first block of each component inside the image's coefficient range
    int32_t blocks_total;
    uint32_t file_size;            // bytes of the file
    int32_t end_on_device;         // the entropy-coded segment's end is still to be found (ke_jpeg_find_end)
};

__constant__ uint8_t c_zigzag[64] = KE_ZZ;

// ---- device bit reader.  One thread per image has nothing to hide memory latency with, and on gfx9 loads and stores share
// one in-order counter (vmcnt): a stream load issued after a coefficient store waits for that store to be acknowledged.  With
// a global store per coefficient and a global load per few symbols the first version of this kernel spent ~1.4 us per
// symbol.  So nothing in the symbol loop touches global memory: the compressed stream is pulled through a 64-byte window per
// lane in LDS (one refill per 56 stream bytes), the coefficients of the current block are collected in LDS and leave as
// eight 16-byte stores per block, the Huffman tables and the zigzag map live in LDS.
constexpr int kWin = 64;                  // stream window per lane (bytes)
constexpr int kWinPitch = kWin + 4;       // + one dword: consecutive lanes start in consecutive banks
constexpr int kBlkPitch = 128 + 16;       // one block of int16 coefficients per lane, rows kept 16-byte aligned

struct Stream {
    const uint8_t *file;                  // global
    uint8_t *win;                         // this lane's LDS window
    uint32_t win_pos;                     // stream position of win[0] (multiple of 4 relative to the file start)
    uint32_t end;
};

__device__ __forceinline__ void stream_load(Stream &s, uint32_t pos) {
    s.win_pos = pos & ~3u;
    const uint8_t *src = s.file + s.win_pos;
#pragma unroll
    for (int k = 0; k < kWin / 4; ++k) {                                  // the file buffer is padded: reads past `end` stay inside it
        uint32_t w;
        __builtin_memcpy(&w, src + 4 * k, 4);
        reinterpret_cast<uint32_t *>(s.win)[k] = w;
    }
}

__device__ __forceinline__ uint32_t stream_byte(Stream &s, uint32_t pos) {
    if (pos - s.win_pos >= (uint32_t)kWin) stream_load(s, pos);
    return s.win[pos - s.win_pos];
}

// four stream bytes from `pos` on, as a little-endian dword (pos + 4 <= end)
__device__ __forceinline__ uint32_t stream_dword(Stream &s, uint32_t pos) {
    if (pos - s.win_pos > (uint32_t)(kWin - 8)) stream_load(s, pos);
    const uint32_t o = pos - s.win_pos;
    const uint32_t *w = reinterpret_cast<const uint32_t *>(s.win) + (o >> 2);
    return __builtin_amdgcn_alignbyte(w[1], w[0], o & 3);
}

__device__ __forceinline__ void bits_fill(KeBits &b, Stream &s) {
    while (b.n <= 32) {
        if (b.marker == 0 && b.pos + 4 <= b.end) {
            const uint32_t w = stream_dword(s, b.pos);
            const uint32_t x = ~w;
            if (((x - 0x01010101u) & ~x & 0x80808080u) == 0) {           // no byte of w is 0xFF
                b.acc |= (uint64_t)__builtin_bswap32(w) << (32 - b.n);
                b.n += 32;
                b.pos += 4;
                continue;
            }
        }
        // one byte, the careful way (ke_bits_fill's body for a single byte)
        uint32_t byte = 0;
        if (b.marker == 0 && b.pos < b.end) {
            byte = stream_byte(s, b.pos);
            if (byte == 0xFF) {
                const uint32_t next = b.pos + 1 < b.end ? stream_byte(s, b.pos + 1) : 0xD9u;
                if (next == 0) {
                    b.pos += 2;
                } else {
                    b.marker = (int32_t)next;
                    byte = 0;
                    b.overrun += 1;
                }
            } else {
                b.pos += 1;
            }
        } else {
            b.overrun += 1;
        }
        b.acc |= (uint64_t)byte << (56 - b.n);
        b.n += 8;
    }
}

template <typename T>
__device__ __forceinline__ int huff_decode(KeBits &b, Stream &st, const T *t) {
    bits_fill(b, st);
    const uint32_t look = t->look[ke_bits_peek(b, 9)];
    if (look) {
        ke_bits_skip(b, (int)(look >> 8));
        return (int)(look & 0xFF);
    }
    int32_t code = (int32_t)ke_bits_peek(b, 10);
    int l = 10;
    while (l <= 16 && code > t->maxcode[l]) {
        ++l;
        code = (int32_t)ke_bits_peek(b, l);
    }
    if (l > 16) return -1;
    ke_bits_skip(b, l);
    return t->huffval[(code + t->valoffset[l]) & 0xFF];
}

// the `s` bits behind a Huffman symbol: huff_decode's fill left more than 32 bits, the code took at most 16, s <= 15
__device__ __forceinline__ int receive_extend(KeBits &b, Stream &, int s) {
    const int v = s ? (int)ke_bits_peek(b, s) : 0;
    ke_bits_skip(b, s);
    return s == 0 ? 0 : (v < (1 << (s - 1)) ? v - (1 << s) + 1 : v);
}

constexpr int kColourRows = 32;    // rows of a workgroup of ke_jpeg_colour
constexpr int kLdsTables = 4;      // distinct Huffman tables a workgroup keeps in LDS (a standard-table file uses four)

// One thread per image.  Coefficients are stored as decoded (int16, natural order, every block written whole); the IDCT kernel
// dequantises.
// ---- the end of a sequential file's entropy-coded segment, found where the bytes are.  ke_jpeg_segment_end's rule: the first
// position e >= scan_offset, e <= size - 2, with p[e] == 0xFF and p[e + 1] neither 0x00 nor RSTn; none = truncated (Pillow
// raises: KE_JPEG_CORRUPT); the marker there must be EOI (anything else = another scan or table: KE_JPEG_UNSUPPORTED).  One wave
// per file, 16 bytes per lane and step; also sets every image's status to the verdict (0 for files the host has walked).
__global__ __launch_bounds__(64) void ke_jpeg_find_end(KeJpegDev *__restrict__ imgs, int64_t n, const uint8_t *__restrict__ files,
                                                       int32_t *__restrict__ status) {
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    if (i >= n) return;
    KeJpegDev &d = imgs[i];
    if (!d.end_on_device) {
        if (lane == 0) status[i] = KE_JPEG_OK;
        return;
    }
    const uint8_t *p = files + d.file_off;
    const uint32_t size = d.file_size, from = d.info.scan_offset;
    // dword-aligned reads: the buffer starts on 256 bytes and ends with 256 bytes of slack
    const uintptr_t a0 = (uintptr_t)(p + from) & ~(uintptr_t)3;
    const int64_t pos0 = (int64_t)(a0 - (uintptr_t)p);            // file position of the first byte read (from - 3 .. from)
    uint32_t found = 0xFFFFFFFFu;
    for (int64_t base = pos0; base + 1 < (int64_t)size; base += 64 * 16) {
        const int64_t q = base + (int64_t)lane * 16;               // this lane's 16 positions q .. q + 15
        uint32_t hit = 0xFFFFFFFFu;
        if (q + 1 < (int64_t)size) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(p + q);
            uint32_t v[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) v[k] = w[k];
#pragma unroll
            for (int k = 15; k >= 0; --k) {
                const uint32_t b0 = (v[k >> 2] >> (8 * (k & 3))) & 0xFFu, b1 = (v[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xFFu;
                const int64_t e = q + k;
                if (b0 == 0xFFu && b1 != 0u && !(b1 >= 0xD0u && b1 <= 0xD7u) && e >= (int64_t)from && e + 1 < (int64_t)size) hit = (uint32_t)e;
            }
        }
        const uint64_t any = __ballot(hit != 0xFFFFFFFFu);
        if (any) {
            found = __shfl(hit, __ffsll((long long)any) - 1);       // lanes hold ascending positions: the first lane's is the first
            break;
        }
    }
    if (lane == 0) {
        if (found == 0xFFFFFFFFu) {
            status[i] = KE_JPEG_CORRUPT;
        } else if (p[found + 1] != 0xD9) {
            status[i] = KE_JPEG_UNSUPPORTED;
        } else {
            d.info.scan_end = found;
            status[i] = KE_JPEG_OK;
        }
    }
}

// ---- restart intervals on separate lanes (KE_JPEG_SPLIT_RESTARTS; ke_jpeg_restarts.h has the plan, the rule and the argument
// why the answers are the walk's).  A file the host found worth splitting (sequential, DRI, a plan of two lanes or more):
struct KeRstFile {
    uint32_t img;                  // its record in the sub-batch
    uint32_t lane_base;            // its first lane among the sub-batch's (a prefix sum of n_lanes); also its slice of the marker table
    KeRstPlan plan;
};

// How a split file is kept from ke_jpeg_entropy without touching that kernel: ke_jpeg_find_restarts sets the DEVICE record's
// info.progressive to kTakenByLanes, and the walk takes files with progressive == 0 only (nothing else on the device reads the
// field: the progressive kernel gets its files as a list from the host).  A flag array as one more parameter of the walk was
// tried first: the same registers and an MCU loop instruction for instruction the parent's, behind 15 more instructions of
// prologue -- and 3.5 % slower on every row with the variable unset, in turns with the parent's build.
constexpr int32_t kTakenByLanes = 2;

// One wave per such file, behind ke_jpeg_find_end (scan_end is known): ke_rst_index a wave wide.  16 bytes per lane and step,
// dword reads as in ke_jpeg_find_end; a lane's markers are counted, the counts' prefix over the wave comes from one __ballot
// per bit of the count, and a running base carries the ordinal from step to step.  marks[lane_base + j] = position of marker
// j * g - 1 (the one lane j starts behind); split[img] = 1 only if the rule holds.
__global__ __launch_bounds__(64) void ke_jpeg_find_restarts(KeJpegDev *__restrict__ imgs, const KeRstFile *__restrict__ rfiles, int64_t n_files,
                                                            const uint8_t *__restrict__ files, const int32_t *__restrict__ status,
                                                            uint32_t *__restrict__ marks, int32_t *__restrict__ split) {
    const int64_t f = blockIdx.x;
    const int lane = threadIdx.x;
    if (f >= n_files) return;
    const KeRstFile rf = rfiles[f];
    if (status[rf.img] != KE_JPEG_OK) return;                       // (split[] was zeroed) turned down by ke_jpeg_find_end
    KeJpegDev &d = imgs[rf.img];
    const uint8_t *p = files + d.file_off;
    const int64_t from = d.info.scan_offset, to = (int64_t)d.info.scan_end - 1;      // markers lie in [from, to)
    const uintptr_t a0 = (uintptr_t)(p + from) & ~(uintptr_t)3;
    const int64_t pos0 = (int64_t)(a0 - (uintptr_t)p);
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t *my_marks = marks + rf.lane_base;
    uint32_t seen = 0;                                              // markers in front of this step (the same in every lane)
    bool bad = false;
    for (int64_t base = pos0; base < to; base += 64 * 16) {
        const int64_t q = base + (int64_t)lane * 16;
        uint32_t v[5] = {0, 0, 0, 0, 0};
        uint32_t hits = 0;                                          // bit k: a marker at q + k
        if (q < to) {                                               // reads q .. q + 19 < scan_end + 19: inside the buffer's 256 bytes of slack
            const uint32_t *w = reinterpret_cast<const uint32_t *>(p + q);
#pragma unroll
            for (int k = 0; k < 5; ++k) v[k] = w[k];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t b0 = (v[k >> 2] >> (8 * (k & 3))) & 0xFFu, b1 = (v[(k + 1) >> 2] >> (8 * ((k + 1) & 3))) & 0xFFu;
                const int64_t e = q + k;
                if (b0 == 0xFFu && b1 != 0u && e >= from && e < to) hits |= 1u << k;
            }
        }
        if (__ballot(hits != 0) == 0) continue;
        const uint32_t mine = (uint32_t)__builtin_popcount(hits);  // 0 .. 8 (two bytes each)
        uint32_t before = 0, step_total = 0;
#pragma unroll
        for (int bit = 0; bit < 4; ++bit) {
            const uint64_t m = __ballot((mine >> bit) & 1u);
            before += (uint32_t)__builtin_popcountll(m & below) << bit;
            step_total += (uint32_t)__builtin_popcountll(m) << bit;
        }
        uint32_t ord = seen + before;
        while (hits) {
            const int k = __builtin_ctz(hits);
            hits &= hits - 1;
            if (p[q + k + 1] != 0xD0u + (ord & 7u)) bad = true;   // (markers are rare: a byte load, no indexing of v by a variable)
            const uint32_t j = (ord + 1) / rf.plan.g;
            if ((ord + 1) % rf.plan.g == 0 && j >= 1 && j < rf.plan.n_lanes) my_marks[j] = (uint32_t)(q + k);
            ++ord;
        }
        seen += step_total;
    }
    const bool any_bad = __ballot(bad) != 0;
    if (lane == 0 && !any_bad && seen == rf.plan.n_int - 1) {
        split[rf.img] = 1;
        d.info.progressive = kTakenByLanes;                         // ke_jpeg_entropy walks files with progressive == 0 only
    }
}

__global__ __launch_bounds__(64) void ke_jpeg_entropy(const KeJpegDev *__restrict__ imgs, int64_t n, const uint8_t *__restrict__ files,
                                                      const KeHuffTable *__restrict__ tables, int16_t *__restrict__ coefs,
                                                      int32_t *__restrict__ status, int lanes) {
    __shared__ KeHuffTable s_tab[kLdsTables];
    __shared__ int s_ids[kLdsTables];
    __shared__ int s_count, s_all;
    __shared__ uint8_t s_zz[64];
    __shared__ __attribute__((aligned(16))) uint8_t s_win[64 * kWinPitch];
    __shared__ __attribute__((aligned(16))) uint8_t s_blk[64 * kBlkPitch];
    const int lane = threadIdx.x;
    // `lanes` images per wave (the rest of the wave idles): a wave pays the largest block of its lanes at every block, so while
    // there are SIMDs to spare a batch is spread over more, narrower waves
    const int64_t i = (int64_t)blockIdx.x * lanes + lane;
    const KeJpegDev &d = imgs[i < n ? i : n - 1];
    const KeJpegInfo &in = d.info;
    // progressive files are ke_jpeg_entropy_prog's; a file ke_jpeg_find_end has turned down keeps that status
    const bool live = lane < lanes && i < n && !in.progressive && status[i] == KE_JPEG_OK;
    // the workgroup's distinct tables (files of one encoder share them): up to four go to LDS
    if (lane == 0) { s_count = 0; s_all = 1; }
    s_zz[lane] = c_zigzag[lane];
    __syncthreads();
    int my_dc[3], my_ac[3];
    for (int c = 0; c < 3; ++c) { my_dc[c] = in.huff_dc[c < in.ncomp ? c : 0]; my_ac[c] = in.huff_ac[c < in.ncomp ? c : 0]; }
    for (int turn = 0; turn < 64; ++turn) {                               // lanes register their ids one after the other
        if (lane == turn && live) {
            for (int c = 0; c < in.ncomp; ++c)
                for (int id : {my_dc[c], my_ac[c]}) {
                    bool found = false;
                    for (int k = 0; k < s_count; ++k) found |= s_ids[k] == id;
                    if (!found) {
                        if (s_count < kLdsTables) s_ids[s_count++] = id; else s_all = 0;
                    }
                }
        }
        __syncthreads();
    }
    const int n_tab = s_count;
    const bool in_lds = s_all != 0;
    if (in_lds) {
        for (int k = 0; k < n_tab; ++k) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(&tables[s_ids[k]]);
            uint32_t *dst = reinterpret_cast<uint32_t *>(&s_tab[k]);
            for (int w = lane; w < (int)(sizeof(KeHuffTable) / 4); w += 64) dst[w] = src[w];
        }
    }
    __syncthreads();
    if (!live) return;
    auto slot_of = [&](int id) { int k = 0; while (k < n_tab - 1 && s_ids[k] != id) ++k; return k; };
    int dc_slot[3], ac_slot[3];
    for (int c = 0; c < 3; ++c) { dc_slot[c] = in_lds ? slot_of(my_dc[c]) : 0; ac_slot[c] = in_lds ? slot_of(my_ac[c]) : 0; }

    KeBits bits;
    ke_bits_init(bits, files + d.file_off, in.scan_offset, in.scan_end);
    Stream st;
    st.file = files + d.file_off;
    st.win = s_win + lane * kWinPitch;
    st.end = in.scan_end;
    stream_load(st, in.scan_offset);
    int16_t *lblk = reinterpret_cast<int16_t *>(s_blk + lane * kBlkPitch);
    const int ncomp = in.ncomp, mcus_x = in.mcus_x, mcus_y = in.mcus_y, restart_interval = in.restart_interval;
    int hs[3], vs[3], bpr[3], bbase[3];
    for (int c = 0; c < 3; ++c) { hs[c] = in.hs[c]; vs[c] = in.vs[c]; bpr[c] = in.plane_w[c] >> 3; bbase[c] = d.block_base[c]; }
    int pred[3] = {0, 0, 0};
    int restart_left = restart_interval;
    int rc = KE_JPEG_OK;
    int16_t *base = coefs + d.coef_off;
    for (int my = 0; my < mcus_y && rc == KE_JPEG_OK; ++my) {
        for (int mx = 0; mx < mcus_x && rc == KE_JPEG_OK; ++mx) {
            if (restart_interval && restart_left == 0) {
                if (ke_bits_restart(bits) != KE_JPEG_OK) { rc = KE_JPEG_CORRUPT; break; }
                pred[0] = pred[1] = pred[2] = 0;
                restart_left = restart_interval;
            }
            for (int c = 0; c < ncomp && rc == KE_JPEG_OK; ++c) {
                const KeHuffTable *gdc = &tables[my_dc[c]], *gac = &tables[my_ac[c]];
                const KeHuffTable *ldc = &s_tab[dc_slot[c]], *lac = &s_tab[ac_slot[c]];
                for (int by = 0; by < vs[c] && rc == KE_JPEG_OK; ++by) {
                    for (int bx = 0; bx < hs[c]; ++bx) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) reinterpret_cast<uint4 *>(lblk)[k] = uint4{0u, 0u, 0u, 0u};
                        int s = in_lds ? huff_decode(bits, st, ldc) : huff_decode(bits, st, gdc);
                        if (s < 0 || s > 11) { rc = KE_JPEG_CORRUPT; break; }
                        pred[c] += receive_extend(bits, st, s);
                        lblk[0] = (int16_t)pred[c];
                        for (int k = 1; k < 64;) {
                            const int rs = in_lds ? huff_decode(bits, st, lac) : huff_decode(bits, st, gac);
                            if (rs < 0) { rc = KE_JPEG_CORRUPT; break; }
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;
                                k += 16;
                                continue;
                            }
                            k += r;
                            if (k > 63) { rc = KE_JPEG_CORRUPT; break; }
                            lblk[k] = (int16_t)receive_extend(bits, st, s);         // zigzag order in memory (ke_jpeg_idct undoes it)
                            ++k;
                        }
                        if (rc != KE_JPEG_OK) break;
                        uint4 *dst = reinterpret_cast<uint4 *>(base + ((size_t)bbase[c] + (size_t)(my * vs[c] + by) * bpr[c] + (mx * hs[c] + bx)) * 64);
#pragma unroll
                        for (int k = 0; k < 8; ++k) dst[k] = reinterpret_cast<const uint4 *>(lblk)[k];
                    }
                }
            }
            --restart_left;
        }
    }
    if (rc == KE_JPEG_OK && ke_bits_ran_dry(bits)) rc = KE_JPEG_CORRUPT;    // used bits beyond the data: truncated or damaged
    status[i] = rc;
}

// One thread per (file, lane j of its plan): global lane L of the sub-batch's n_lanes_total belongs to the file whose
// [lane_base, lane_base + n_lanes) holds it (binary search: consecutive lanes are mostly one file's, so a wave's lanes share
// their Huffman tables in LDS).  The machinery is ke_jpeg_entropy's -- stream window, block in LDS, tables in LDS, `lanes` per
// wave -- and so is the MCU loop, as a second copy: here it runs over a range of MCUs behind a start that is not the scan's,
// and the walk's loop is left as it stands (DESIGN 5 has the register counts).  Only a failing lane writes the file's status,
// and all of them write the same value.
__global__ __launch_bounds__(64) void ke_jpeg_entropy_rst(const KeJpegDev *__restrict__ imgs, const KeRstFile *__restrict__ rfiles, int64_t n_files,
                                                          int64_t n_lanes_total, const uint8_t *__restrict__ files,
                                                          const KeHuffTable *__restrict__ tables, int16_t *__restrict__ coefs,
                                                          int32_t *__restrict__ status, int lanes, const uint32_t *__restrict__ marks,
                                                          const int32_t *__restrict__ split) {
    __shared__ KeHuffTable s_tab[kLdsTables];
    __shared__ int s_ids[kLdsTables];
    __shared__ int s_count, s_all;
    __shared__ __attribute__((aligned(16))) uint8_t s_win[64 * kWinPitch];
    __shared__ __attribute__((aligned(16))) uint8_t s_blk[64 * kBlkPitch];
    const int lane = threadIdx.x;
    const int64_t L = (int64_t)blockIdx.x * lanes + lane;
    const int64_t Lc = L < n_lanes_total ? L : n_lanes_total - 1;
    int64_t lo = 0, hi = n_files - 1;                                     // the last file whose lane_base <= Lc
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)rfiles[mid].lane_base <= Lc) lo = mid; else hi = mid - 1;
    }
    const KeRstFile rf = rfiles[lo];
    const KeJpegDev &d = imgs[rf.img];
    const KeJpegInfo &in = d.info;
    const uint32_t j = (uint32_t)(Lc - rf.lane_base);
    const bool live = lane < lanes && L < n_lanes_total && j < rf.plan.n_lanes && split[rf.img] != 0;
    if (lane == 0) { s_count = 0; s_all = 1; }
    __syncthreads();
    int my_dc[3], my_ac[3];
    for (int c = 0; c < 3; ++c) { my_dc[c] = in.huff_dc[c < in.ncomp ? c : 0]; my_ac[c] = in.huff_ac[c < in.ncomp ? c : 0]; }
    for (int turn = 0; turn < 64; ++turn) {                               // lanes register their ids one after the other
        if (lane == turn && live) {
            for (int c = 0; c < in.ncomp; ++c)
                for (int id : {my_dc[c], my_ac[c]}) {
                    bool found = false;
                    for (int k = 0; k < s_count; ++k) found |= s_ids[k] == id;
                    if (!found) {
                        if (s_count < kLdsTables) s_ids[s_count++] = id; else s_all = 0;
                    }
                }
        }
        __syncthreads();
    }
    const int n_tab = s_count;
    const bool in_lds = s_all != 0;
    if (in_lds) {
        for (int k = 0; k < n_tab; ++k) {
            const uint32_t *src = reinterpret_cast<const uint32_t *>(&tables[s_ids[k]]);
            uint32_t *dst = reinterpret_cast<uint32_t *>(&s_tab[k]);
            for (int w = lane; w < (int)(sizeof(KeHuffTable) / 4); w += 64) dst[w] = src[w];
        }
    }
    __syncthreads();
    if (!live) return;
    auto slot_of = [&](int id) { int k = 0; while (k < n_tab - 1 && s_ids[k] != id) ++k; return k; };
    int dc_slot[3], ac_slot[3];
    for (int c = 0; c < 3; ++c) { dc_slot[c] = in_lds ? slot_of(my_dc[c]) : 0; ac_slot[c] = in_lds ? slot_of(my_ac[c]) : 0; }

    const int ncomp = in.ncomp, mcus_x = in.mcus_x, restart_interval = in.restart_interval;
    const KeRstLane ln = ke_rst_lane(rf.plan, (uint32_t)(in.mcus_x * in.mcus_y), (uint32_t)restart_interval, j);
    // the lane's bytes: from 2 behind the marker in front of its first interval to the marker that closes its last
    const uint32_t start = j == 0 ? in.scan_offset : marks[rf.lane_base + j] + 2;
    const uint32_t end = j + 1 == rf.plan.n_lanes ? in.scan_end : marks[rf.lane_base + j + 1];
    KeBits bits;
    ke_bits_init(bits, files + d.file_off, start, end);
    bits.next_rst = (int32_t)ln.next_rst;
    Stream st;
    st.file = files + d.file_off;
    st.win = s_win + lane * kWinPitch;
    st.end = end;
    stream_load(st, start);
    int16_t *lblk = reinterpret_cast<int16_t *>(s_blk + lane * kBlkPitch);
    int hs[3], vs[3], bpr[3], bbase[3];
    for (int c = 0; c < 3; ++c) { hs[c] = in.hs[c]; vs[c] = in.vs[c]; bpr[c] = in.plane_w[c] >> 3; bbase[c] = d.block_base[c]; }
    int pred[3] = {0, 0, 0};
    int restart_left = restart_interval;
    int rc = KE_JPEG_OK;
    int16_t *base = coefs + d.coef_off;
    int my = (int)(ln.mcu_first / (uint32_t)mcus_x), mx = (int)(ln.mcu_first - (uint32_t)my * (uint32_t)mcus_x);
    for (uint32_t m = ln.mcu_first; m < ln.mcu_last && rc == KE_JPEG_OK; ++m) {
        if (restart_left == 0) {
            if (ke_bits_restart(bits) != KE_JPEG_OK) { rc = KE_JPEG_CORRUPT; break; }
            pred[0] = pred[1] = pred[2] = 0;
            restart_left = restart_interval;
        }
        for (int c = 0; c < ncomp && rc == KE_JPEG_OK; ++c) {
            const KeHuffTable *gdc = &tables[my_dc[c]], *gac = &tables[my_ac[c]];
            const KeHuffTable *ldc = &s_tab[dc_slot[c]], *lac = &s_tab[ac_slot[c]];
            for (int by = 0; by < vs[c] && rc == KE_JPEG_OK; ++by) {
                for (int bx = 0; bx < hs[c]; ++bx) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) reinterpret_cast<uint4 *>(lblk)[k] = uint4{0u, 0u, 0u, 0u};
                    int s = in_lds ? huff_decode(bits, st, ldc) : huff_decode(bits, st, gdc);
                    if (s < 0 || s > 11) { rc = KE_JPEG_CORRUPT; break; }
                    pred[c] += receive_extend(bits, st, s);
                    lblk[0] = (int16_t)pred[c];
                    for (int k = 1; k < 64;) {
                        const int rs = in_lds ? huff_decode(bits, st, lac) : huff_decode(bits, st, gac);
                        if (rs < 0) { rc = KE_JPEG_CORRUPT; break; }
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s == 0) {
                            if (r != 15) break;
                            k += 16;
                            continue;
                        }
                        k += r;
                        if (k > 63) { rc = KE_JPEG_CORRUPT; break; }
                        lblk[k] = (int16_t)receive_extend(bits, st, s);         // zigzag order in memory, as ke_jpeg_entropy leaves it
                        ++k;
                    }
                    if (rc != KE_JPEG_OK) break;
                    uint4 *dst = reinterpret_cast<uint4 *>(base + ((size_t)bbase[c] + (size_t)(my * vs[c] + by) * bpr[c] + (mx * hs[c] + bx)) * 64);
#pragma unroll
                    for (int k = 0; k < 8; ++k) dst[k] = reinterpret_cast<const uint4 *>(lblk)[k];
                }
            }
        }
        --restart_left;
        if (++mx == mcus_x) { mx = 0; ++my; }
    }
    // the walk's check at the restart behind this lane's last interval (or at the end of the scan): bits beyond the lane's data
    if (rc == KE_JPEG_OK && ke_bits_ran_dry(bits)) rc = KE_JPEG_CORRUPT;
    if (rc != KE_JPEG_OK) status[rf.img] = rc;
}

// ---- progressive files.  One thread per image again, scan after scan into the image's coefficient array (zeroed before).
// Every scan of such a file comes with its own optimised Huffman tables, so nothing can be shared between lanes or kept from
// scan to scan: a lane builds the canonical form of its scan's tables -- 16 limits, 16 bases, the symbols in code order --
// into its slices of LDS from the DHT bytes of the file (as the PNG kernel does for deflate) and decodes by comparison.
// What a scan writes needs no read-back except in AC refinement scans: first DC / AC scans store coefficients straight to
// HBM, a DC refinement is one atomic OR per block; AC refinement pulls the block into LDS, works there and puts it back.

struct ProgTables {            // per lane: three slots (the components of a DC scan; slot 0 for AC scans)
    uint32_t *lim;             // slot s, dword k (limits of lengths 2k+1 | 2k+2 in halves) at lim[64 * (8 * s + k)]
    uint32_t *base;            // same layout, int16 halves
    uint8_t *sym;              // slot s symbol j at sym[64 * (16 * s + j)] (DC: <= 16 symbols a slot; AC: slot 0, 256)
};

// DHT payload (16 counts, then the symbols) -> canonical form; false when the counts are not a prefix code
__device__ __forceinline__ bool prog_build(const ProgTables &t, int slot, const uint8_t *dht, int max_syms) {
    uint32_t code = 0, off = 0, lw = 0, bw = 0;
    bool ok = true;
    for (int l = 1; l <= 16; ++l) {
        const uint32_t cnt = dht[l - 1];
        const uint32_t b = (off - code) & 0xFFFFu;                 // symbol index = code + base
        code += cnt;
        ok = ok && code <= (1u << l);
        const uint32_t limit = min(code << (16 - l), 0xFFFFu);     // one past the last code of this length, left-aligned
        if (l & 1) { lw = limit; bw = b; } else { t.lim[64 * (8 * slot + (l >> 1) - 1)] = lw | (limit << 16); t.base[64 * (8 * slot + (l >> 1) - 1)] = bw | (b << 16); }
        off += cnt;
        code <<= 1;
    }
    ok = ok && off <= (uint32_t)max_syms;
    const uint32_t n = min(off, (uint32_t)max_syms);
    for (uint32_t j = 0; j < n; ++j) t.sym[64 * (16 * slot + j)] = dht[16 + j];
    return ok;
}

// the reader of ke_prog_*.  AC scans have one table: its limits are taken into registers for the length of the scan (one LDS
// round trip less per symbol); the tables of a DC scan (one per component) stay in LDS, a DC symbol being one per block.
template <bool AC>
struct ProgReader {
    KeBits &b;
    Stream &st;
    const ProgTables &t;
    int sym_mask;              // symbols a slot can hold - 1
    uint32_t l0, l1, l2, l3, l4, l5, l6, l7;
    __device__ __forceinline__ void latch() {
        l0 = t.lim[0]; l1 = t.lim[64]; l2 = t.lim[128]; l3 = t.lim[192]; l4 = t.lim[256]; l5 = t.lim[320]; l6 = t.lim[384]; l7 = t.lim[448];
    }
    __device__ __forceinline__ int sym(int slot) {
        bits_fill(b, st);
        const uint32_t v = ke_bits_peek(b, 16);
        int reached = 0;
        if (AC) {
            slot = 0;
#define KE_REACH(w) reached += (int)(v >= ((w) & 0xFFFFu)) + (int)(v >= ((w) >> 16))
            KE_REACH(l0); KE_REACH(l1); KE_REACH(l2); KE_REACH(l3); KE_REACH(l4); KE_REACH(l5); KE_REACH(l6); KE_REACH(l7);
#undef KE_REACH
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t w = t.lim[64 * (8 * slot + k)];
                reached += (int)(v >= (w & 0xFFFFu)) + (int)(v >= (w >> 16));
            }
        }
        if (reached >= 16) return -1;                              // beyond the last code
        const int len = reached + 1;
        const uint32_t bw = t.base[64 * (8 * slot + (reached >> 1))];
        const int base = (int)(int16_t)((reached & 1) ? bw >> 16 : bw & 0xFFFFu);
        ke_bits_skip(b, len);
        return t.sym[64 * (16 * slot + (((int)(v >> (16 - len)) + base) & sym_mask))];
    }
    __device__ __forceinline__ uint32_t bits(int k) {
        bits_fill(b, st);
        const uint32_t v = ke_bits_peek(b, k);
        ke_bits_skip(b, k);
        return v;
    }
    __device__ __forceinline__ int bit() { return (int)bits(1); }
};

struct StoreBlock {            // a block that is only written: coefficients go straight to HBM
    int16_t *g;
    struct Ref {
        int16_t *p;
        __device__ __forceinline__ void operator=(int16_t v) { *p = v; }
    };
    __device__ __forceinline__ Ref operator[](int pos) const { return Ref{g + pos}; }
};

// ke_prog_ac_refine (ke_jpeg_core.h; jdphuff.c decode_mcu_AC_refine) for a block in zigzag order whose nonzero coefficients are
// known as a bit mask (`nz`, bit k = position k): the reference form visits every position of the band -- 63 LDS reads per block
// with all 64 lanes in step, and the refinement scans were 83 of the 88 ms of a 16 384-file batch's entropy decoding -- while the
// work is per NONZERO coefficient (a correction bit each) and per symbol (skip r zeros: bit arithmetic on the mask).  Same
// bits read in the same order, same coefficients written.
template <typename Rd>
__device__ __forceinline__ int prog_ac_refine_masked(Rd &rd, int16_t *blk, uint64_t nz, int ss, int se, int al, uint32_t &eobrun) {
    const int p1 = 1 << al, m1 = -(1 << al);
    const uint64_t band = ((se >= 63 ? 0ull : (1ull << (se + 1))) - 1ull) & ~((1ull << ss) - 1ull);
    uint64_t ahead_nz = nz & band, ahead_z = ~nz & band;             // positions of the band not yet passed
    auto correct = [&](uint64_t which) {                             // one more bit for each of these (nonzero) coefficients, in order
        while (which) {
            const int pos = __builtin_ctzll(which);
            which &= which - 1;
            const int c = blk[pos];
            if (rd.bit() && (c & p1) == 0) blk[pos] = (int16_t)(c + (c >= 0 ? p1 : m1));
        }
    };
    if (eobrun == 0) {
        int k = ss;
        while (k <= se) {
            const int rs = rd.sym(0);
            if (rs < 0) return KE_JPEG_CORRUPT;
            const int r = rs >> 4;
            int s = rs & 15;
            if (s) {
                s = rd.bit() ? p1 : m1;                      // the size of a new coefficient is always 1; its sign follows
            } else if (r != 15) {
                eobrun = 1u << r;
                if (r) eobrun += rd.bits(r);
                break;                                       // the rest of the band belongs to the end-of-band run
            }
            // the position the reference loop stops at: the (r + 1)-th zero still ahead, or just behind the band
            uint64_t z = ahead_z;
            for (int q = 0; q < r && z; ++q) z &= z - 1;
            const int t = z ? __builtin_ctzll(z) : se + 1;
            const uint64_t upto = t >= 63 ? ~0ull : (1ull << (t + 1)) - 1ull;      // positions 0 .. t
            correct(ahead_nz & upto);                        // (position t itself is a zero, or lies behind the band)
            ahead_nz &= ~upto;
            ahead_z &= ~upto;
            if (s) {
                if (t > 63) return KE_JPEG_CORRUPT;
                blk[t] = (int16_t)s;
            }
            k = t + 1;
        }
    }
    if (eobrun > 0) {
        correct(ahead_nz);
        --eobrun;
    }
    return KE_JPEG_OK;
}

__global__ __launch_bounds__(64) void ke_jpeg_entropy_prog(const KeJpegDev *__restrict__ imgs, const int32_t *__restrict__ list, int64_t n,
                                                           const uint8_t *__restrict__ files, const KeJpegScan *__restrict__ scans,
                                                           int16_t *__restrict__ coefs, int32_t *__restrict__ status, int lanes) {
    __shared__ uint32_t s_lim[24 * 64], s_base[24 * 64];
    __shared__ uint8_t s_sym[256 * 64];
    __shared__ uint8_t s_zz[64];
    __shared__ __attribute__((aligned(16))) uint8_t s_win[64 * kWinPitch];
    __shared__ __attribute__((aligned(16))) uint8_t s_blk[64 * kBlkPitch];
    const int lane = threadIdx.x;
    s_zz[lane] = (uint8_t)lane;            // the blocks are kept in zigzag order (ke_jpeg_idct undoes it): position k is element k
    __syncthreads();
    const int64_t slot_i = (int64_t)blockIdx.x * lanes + lane;
    if (lane >= lanes || slot_i >= n) return;
    const int32_t i = list[slot_i];
    const KeJpegDev &d = imgs[i];
    const KeJpegInfo &in = d.info;
    const uint8_t *file = files + d.file_off;
    ProgTables tab{s_lim + lane, s_base + lane, s_sym + lane};
    Stream st;
    st.file = file;
    st.win = s_win + lane * kWinPitch;
    int16_t *lblk = reinterpret_cast<int16_t *>(s_blk + lane * kBlkPitch);
    int16_t *base = coefs + d.coef_off;
    int rc = KE_JPEG_OK;
    for (int si = 0; si < in.nscans && rc == KE_JPEG_OK; ++si) {
        const KeJpegScan &sc = scans[in.first_scan + si];
        const int ss = sc.ss, se = sc.se, ah = sc.ah, al = sc.al, ns = sc.ncomp, ri = sc.restart_interval;
        const bool dc = ss == 0;
        if (!(dc && ah != 0)) {                                      // a DC refinement is raw bits, no table
            for (int k = 0; k < (dc ? ns : 1); ++k)
                if (!prog_build(tab, k, file + (dc ? sc.dc_dht[k] : sc.ac_dht[0]), dc ? 16 : 256)) rc = KE_JPEG_CORRUPT;
            if (rc != KE_JPEG_OK) break;
        }
        KeBits bits;
        ke_bits_init(bits, file, sc.offset, sc.end);
        st.end = sc.end;
        stream_load(st, sc.offset);
        int pred[3] = {0, 0, 0};
        uint32_t eobrun = 0;
        int restart_left = ri;
        if (dc) {
            ProgReader<false> rd{bits, st, tab, 15, 0, 0, 0, 0, 0, 0, 0, 0};
            // MCUs of hs x vs blocks per component when several components share the scan, single blocks otherwise
            const bool inter = ns > 1;
            const int c0 = sc.comp[0];
            const int units_x = inter ? in.mcus_x : (in.comp_w[c0] + 7) >> 3, units_y = inter ? in.mcus_y : (in.comp_h[c0] + 7) >> 3;
            for (int uy = 0; uy < units_y && rc == KE_JPEG_OK; ++uy)
                for (int ux = 0; ux < units_x && rc == KE_JPEG_OK; ++ux) {
                    if (ri && restart_left == 0) {
                        if (ke_bits_restart(bits) != KE_JPEG_OK) { rc = KE_JPEG_CORRUPT; break; }
                        pred[0] = pred[1] = pred[2] = 0;
                        restart_left = ri;
                    }
                    for (int k = 0; k < ns && rc == KE_JPEG_OK; ++k) {
                        const int c = sc.comp[k];
                        const int hs = inter ? in.hs[c] : 1, vs = inter ? in.vs[c] : 1, bpr = in.plane_w[c] >> 3;
                        for (int by = 0; by < vs && rc == KE_JPEG_OK; ++by)
                            for (int bx = 0; bx < hs; ++bx) {
                                int16_t *g = base + ((size_t)d.block_base[c] + (size_t)(uy * vs + by) * bpr + (ux * hs + bx)) * 64;
                                if (ah == 0) {
                                    int v;
                                    if (ke_prog_dc_first(rd, k, pred[k], al, &v) != KE_JPEG_OK) { rc = KE_JPEG_CORRUPT; break; }
                                    g[0] = (int16_t)v;
                                } else if (rd.bit()) {
                                    // coefficient 0 is the low half of the block's first dword: one more bit, no read-back
                                    atomicOr(reinterpret_cast<unsigned int *>(g), 1u << al);
                                }
                            }
                    }
                    --restart_left;
                }
        } else {
            ProgReader<true> rd{bits, st, tab, 255, 0, 0, 0, 0, 0, 0, 0, 0};
            rd.latch();
            const int c = sc.comp[0], bpr = in.plane_w[c] >> 3;
            const int bw = (in.comp_w[c] + 7) >> 3, bh = (in.comp_h[c] + 7) >> 3;
            for (int brow = 0; brow < bh && rc == KE_JPEG_OK; ++brow)
                for (int bcol = 0; bcol < bw; ++bcol) {
                    if (ri && restart_left == 0) {
                        if (ke_bits_restart(bits) != KE_JPEG_OK) { rc = KE_JPEG_CORRUPT; break; }
                        eobrun = 0;
                        restart_left = ri;
                    }
                    int16_t *g = base + ((size_t)d.block_base[c] + (size_t)brow * bpr + bcol) * 64;
                    if (ah == 0) {
                        StoreBlock blk{g};
                        if (ke_prog_ac_first(rd, 0, blk, s_zz, ss, se, al, eobrun) != KE_JPEG_OK) { rc = KE_JPEG_CORRUPT; break; }
                    } else {
                        const uint4 *src = reinterpret_cast<const uint4 *>(g);
                        uint32_t nz_lo = 0, nz_hi = 0;               // which of the 64 coefficients are nonzero, two bits per dword
#pragma unroll
                        for (int k = 0; k < 8; ++k) {
                            const uint4 v = src[k];
                            reinterpret_cast<uint4 *>(lblk)[k] = v;
                            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
                            uint32_t m = 0;
#pragma unroll
                            for (int j = 0; j < 4; ++j) m |= ((uint32_t)((w[j] & 0xFFFFu) != 0) | ((uint32_t)((w[j] >> 16) != 0) << 1)) << (2 * j);
                            if (k < 4) nz_lo |= m << (8 * k); else nz_hi |= m << (8 * (k - 4));
                        }
                        if (prog_ac_refine_masked(rd, lblk, ((uint64_t)nz_hi << 32) | nz_lo, ss, se, al, eobrun) != KE_JPEG_OK) { rc = KE_JPEG_CORRUPT; break; }
                        uint4 *dst = reinterpret_cast<uint4 *>(g);
#pragma unroll
                        for (int k = 0; k < 8; ++k) dst[k] = reinterpret_cast<const uint4 *>(lblk)[k];
                    }
                    --restart_left;
                }
        }
        if (rc == KE_JPEG_OK && ke_bits_ran_dry(bits)) rc = KE_JPEG_CORRUPT;  // used bits beyond the scan's data: truncated or damaged
    }
    status[i] = rc;
}

struct IdctMul24 {                  // see ke_idct_islow: multiplicands below 2^16 wherever the results are used
    static __device__ __forceinline__ int mul(int a, int k) { return __mul24(a, k); }
};

__global__ __launch_bounds__(256) void ke_jpeg_idct(const KeJpegDev *__restrict__ imgs, int64_t n_imgs, const int16_t *__restrict__ coefs,
                                                    uint8_t *__restrict__ planes, int32_t *status) {
    const int64_t img = (int64_t)blockIdx.z * 65535 + blockIdx.y;       // a grid dimension ends at 65535: the image index takes two
    if (img >= n_imgs) return;
    const KeJpegDev &d = imgs[img];
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= d.blocks_total) return;
    const KeJpegInfo &in = d.info;
    int c = 0;
    if (in.ncomp == 3) c = b >= d.block_base[2] ? 2 : (b >= d.block_base[1] ? 1 : 0);
    const int local = b - d.block_base[c];
    const int bpr = in.plane_w[c] >> 3;
    const int brow = local / bpr, bcol = local - brow * bpr;
    const int16_t *src = coefs + d.coef_off + (size_t)b * 64;
    int blk[64];
    // The entropy kernels leave the 64 coefficients in ZIGZAG order (position k of the scan is element k: no table look-up per
    // coefficient there, and the bands of a progressive scan are runs of elements); here every element has a compile-time
    // index, so putting it where the IDCT wants it costs nothing.
    constexpr uint8_t nat[64] = KE_ZZ;
#pragma unroll
    for (int k = 0; k < 8; ++k) {                                        // 128 bytes per block: eight 16-byte loads
        const int4 v = reinterpret_cast<const int4 *>(src)[k];
        const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {                                    // dequantise here: the entropy threads store raw values
            blk[nat[8 * k + 2 * j]] = (int)(int16_t)(w[j] & 0xFFFF) * (int)in.quant[c][nat[8 * k + 2 * j]];
            blk[nat[8 * k + 2 * j + 1]] = (w[j] >> 16) * (int)in.quant[c][nat[8 * k + 2 * j + 1]];
        }
    }
    uint8_t rows[64];
    // a block outside the bound of ke_idct_islow: the file goes back to the caller (unless the entropy decoder already said
    // worse of it; every thread that finds one stores the same value)
    if (!ke_idct_islow<int[64], IdctMul24>(blk, rows, 8) && status[img] == KE_JPEG_OK) status[img] = KE_JPEG_UNSUPPORTED;
    uint8_t *dst = planes + d.plane_off[c] + (size_t)(brow * 8) * in.plane_w[c] + bcol * 8;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        uint2 v;
        v.x = rows[8 * r] | (rows[8 * r + 1] << 8) | (rows[8 * r + 2] << 16) | ((uint32_t)rows[8 * r + 3] << 24);
        v.y = rows[8 * r + 4] | (rows[8 * r + 5] << 8) | (rows[8 * r + 6] << 16) | ((uint32_t)rows[8 * r + 7] << 24);
        *reinterpret_cast<uint2 *>(dst + (size_t)r * in.plane_w[c]) = v;
    }
}

// the four chroma samples around quad x0 (columns i0 - 1 .. i0 + 2) of one row pair, each already weighted 3:1 between the
// nearer and the farther row when the component is subsampled vertically: two dword loads.  No clamping of the columns: the
// callers' edge cases (jdsample.c's first / last column) never use the samples that would lie outside the component -- at
// i0 = 0 the load starts at column 0 and the bytes move up one place, c[0] unused; at the right edge c[2] / c[3] are unused.
__device__ __forceinline__ void chroma4(const uint8_t *in0, const uint8_t *in1, int i0, bool v2, int *c) {
    const bool first = i0 == 0;
    uint32_t a, b;
    __builtin_memcpy(&a, in0 + (first ? 0 : i0 - 1), 4);      // bytes from..from+3 lie inside the padded plane row
    __builtin_memcpy(&b, in1 + (first ? 0 : i0 - 1), 4);      // (aligned dwords + a funnel shift instead: no faster, 14.0 against 13.7 ms)
    a = first ? a << 8 : a;
    b = first ? b << 8 : b;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int s0 = (int)((a >> (8 * j)) & 255u), s1 = (int)((b >> (8 * j)) & 255u);
        c[j] = v2 ? s0 * 3 + s1 : s0;
    }
}

__device__ __forceinline__ int4 upsample4_fast(const uint8_t *plane, int pw, int cw, int ch, int hfac, int vfac, int x0, int y) {
    if (hfac == 1 && vfac == 2) {                             // 4:4:0 (h1v2_fancy_upsample): two dwords, 3:1 between the rows
        const int r0 = y >> 1;
        int r1 = (y & 1) ? r0 + 1 : r0 - 1;
        r1 = r1 < 0 ? 0 : (r1 > ch - 1 ? ch - 1 : r1);
        const uint32_t a = *reinterpret_cast<const uint32_t *>(plane + (__umul24(r0, pw) + (uint32_t)x0));
        const uint32_t b = *reinterpret_cast<const uint32_t *>(plane + (__umul24(r1, pw) + (uint32_t)x0));
        const int bias = (y & 1) ? 2 : 1;
        return make_int4((int)((a & 255u) * 3u + (b & 255u) + bias) >> 2, (int)(((a >> 8) & 255u) * 3u + ((b >> 8) & 255u) + bias) >> 2,
                         (int)(((a >> 16) & 255u) * 3u + ((b >> 16) & 255u) + bias) >> 2, (int)((a >> 24) * 3u + (b >> 24) + bias) >> 2);
    }
    if (hfac == 1) {                                          // the samples themselves, x0 a multiple of 4
        const uint32_t v = *reinterpret_cast<const uint32_t *>(plane + (__umul24(y, pw) + (uint32_t)x0));
        return make_int4((int)(v & 255u), (int)((v >> 8) & 255u), (int)((v >> 16) & 255u), (int)(v >> 24));
    }
    if (cw <= 2) {
        int t[4];
        ke_upsample4(plane, pw, cw, ch, hfac, vfac, x0, y, t);
        return make_int4(t[0], t[1], t[2], t[3]);
    }
    const int i0 = x0 >> 1;
    const int r0 = vfac == 2 ? (y >> 1) : y;
    int r1 = r0;
    if (vfac == 2) {
        r1 = (y & 1) ? r0 + 1 : r0 - 1;
        r1 = r1 < 0 ? 0 : (r1 > ch - 1 ? ch - 1 : r1);
    }
    int c[4];
    chroma4(plane + __umul24(r0, pw), plane + __umul24(r1, pw), i0, vfac == 2, c);      // rows and widths are far below 2^24
    const bool first = i0 == 0, last0 = i0 == cw - 1, last1 = i0 + 1 >= cw - 1;
    if (vfac == 2)
        return make_int4(first ? (c[1] * 4 + 8) >> 4 : (c[1] * 3 + c[0] + 8) >> 4, last0 ? (c[1] * 4 + 7) >> 4 : (c[1] * 3 + c[2] + 7) >> 4,
                         (c[2] * 3 + c[1] + 8) >> 4, last1 ? (c[2] * 4 + 7) >> 4 : (c[2] * 3 + c[3] + 7) >> 4);
    return make_int4(first ? c[1] : (c[1] * 3 + c[0] + 1) >> 2, last0 ? c[1] : (c[1] * 3 + c[2] + 2) >> 2, (c[2] * 3 + c[1] + 1) >> 2,
                     last1 ? c[2] : (c[2] * 3 + c[3] + 2) >> 2);
}

// jdcolor.c ycc_rgb_convert for one pixel, as R | G << 8 | B << 16
// a * k + c on the 24-bit multiplier (full rate; a 32-bit multiply takes four times as long).  Spelled out because the compiler
// rewrites __mul24 on operands it can bound into a plain multiply and then picks the 32-bit instruction for it.
__device__ __forceinline__ int mad24(int a, int k, int c) {
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(k), "v"(c));
    return r;
}

__device__ __forceinline__ uint32_t ycc_to_rgb24(int y, int cb, int cr) {
    // the chroma offset of 128 folded into the rounding constant: k * (c - 128) + 32768 = k * c + (32768 - 128 k) exactly
    const int r = y + (mad24(cr, 91881, 32768 - 128 * 91881) >> 16);
    const int g = y + (mad24(cr, -46802, mad24(cb, -22554, 32768 + 128 * 22554 + 128 * 46802)) >> 16);
    const int b = y + (mad24(cb, 116130, 32768 - 128 * 116130) >> 16);
    return (uint32_t)min(max(r, 0), 255) | ((uint32_t)min(max(g, 0), 255) << 8) | ((uint32_t)min(max(b, 0), 255) << 16);
}

__global__ __launch_bounds__(256) void ke_jpeg_colour(const KeJpegDev *__restrict__ imgs, int64_t n_imgs, int xblocks,
                                                      const uint8_t *__restrict__ planes, uint8_t *__restrict__ out) {
    // A workgroup takes 256 columns of kColourRows rows, four rows at a time (65 536 images of 512 x 512 are 16.7 M groups of
    // four rows: one workgroup each was bound by the rate workgroups can be started at); the turns are independent, so their
    // loads overlap.
    const int64_t img = (int64_t)blockIdx.z * 65535 + blockIdx.y;       // image over two grid dimensions, (column, row) blocks in x
    if (img >= n_imgs) return;
    const KeJpegDev &d = imgs[img];
    const KeJpegInfo &in = d.info;
    const int r = threadIdx.x >> 6, q = threadIdx.x & 63;
    const int block_x = (int)(blockIdx.x % (unsigned)xblocks), block_y = (int)(blockIdx.x / (unsigned)xblocks);
    const int x0 = block_x * 256 + q * 4;
    if (x0 >= in.width) return;
    const uint8_t *Y = planes + d.plane_off[0], *Cb = planes + d.plane_off[1], *Cr = planes + d.plane_off[2];
    uint8_t *dst = out + d.out_off;
    const int npx = min(4, in.width - x0);
#pragma unroll 4
    for (int turn = 0; turn < kColourRows / 4; ++turn) {
        const int y = block_y * kColourRows + turn * 4 + r;
        if (y >= in.height) break;
        // four luma samples in one load (plane rows are multiples of 8 bytes, x0 of 4)
        const uint32_t y4 = *reinterpret_cast<const uint32_t *>(Y + (__umul24(y, in.plane_w[0]) + (uint32_t)x0));
        if (in.ncomp == 1) {
            uint8_t *o = dst + (size_t)y * in.width + x0;
            if (npx == 4) __builtin_memcpy(o, &y4, 4);
            else for (int k = 0; k < npx; ++k) o[k] = (uint8_t)(y4 >> (8 * k));
            continue;
        }
        const int4 cb = upsample4_fast(Cb, in.plane_w[1], in.comp_w[1], in.comp_h[1], in.hmax, in.vmax, x0, y);
        const int4 cr = upsample4_fast(Cr, in.plane_w[2], in.comp_w[2], in.comp_h[2], in.hmax, in.vmax, x0, y);
        const uint32_t p0 = ycc_to_rgb24((int)(y4 & 0xFF), cb.x, cr.x), p1 = ycc_to_rgb24((int)((y4 >> 8) & 0xFF), cb.y, cr.y);
        const uint32_t p2 = ycc_to_rgb24((int)((y4 >> 16) & 0xFF), cb.z, cr.z), p3 = ycc_to_rgb24((int)(y4 >> 24), cb.w, cr.w);
        const uint32_t w0 = p0 | (p1 << 24), w1 = (p1 >> 8) | (p2 << 16), w2 = (p2 >> 16) | (p3 << 8);
        uint8_t *o = dst + (size_t)(__umul24(y, in.width) + (uint32_t)x0) * 3;
        if (npx == 4) {
            typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
            const u32x3 w{w0, w1, w2};
            __builtin_memcpy(o, &w, 12);                                  // one 12-byte store, any alignment (rows of 3*width bytes)
        } else {
            for (int k = 0; k < 3 * npx; ++k) o[k] = (uint8_t)((k < 4 ? w0 : k < 8 ? w1 : w2) >> (8 * (k & 3)));
        }
    }
}

// ---- reduced-size decoding (ke_jpeg_decode_scaled): the coefficients are those of the full-size decode; each component's
// blocks go through the transform of its size at the file's scale (ke_jpeg_core.h, KeJpegScaled) into planes of that size,
// and upsampling and colour run over the reduced image.  Planes lie where the full-size ones would (they are smaller).
__global__ __launch_bounds__(256) void ke_jpeg_idct_scaled(const KeJpegDev *__restrict__ imgs, const KeJpegScaled *__restrict__ geo, int64_t n_imgs,
                                                           const int16_t *__restrict__ coefs, uint8_t *__restrict__ planes, int32_t *status) {
    const int64_t img = (int64_t)blockIdx.z * 65535 + blockIdx.y;
    if (img >= n_imgs) return;
    const KeJpegDev &d = imgs[img];
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= d.blocks_total) return;
    const KeJpegInfo &in = d.info;
    const KeJpegScaled &g = geo[img];
    int c = 0;
    if (in.ncomp == 3) c = b >= d.block_base[2] ? 2 : (b >= d.block_base[1] ? 1 : 0);
    const int local = b - d.block_base[c];
    const int bpr = in.plane_w[c] >> 3;
    const int brow = local / bpr, bcol = local - brow * bpr;
    const int16_t *src = coefs + d.coef_off + (size_t)b * 64;
    int blk[64];
    constexpr uint8_t nat[64] = KE_ZZ;                                   // zigzag order in memory, as for ke_jpeg_idct
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int4 v = reinterpret_cast<const int4 *>(src)[k];
        const int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            blk[nat[8 * k + 2 * j]] = (int)(int16_t)(w[j] & 0xFFFF) * (int)in.quant[c][nat[8 * k + 2 * j]];
            blk[nat[8 * k + 2 * j + 1]] = (w[j] >> 16) * (int)in.quant[c][nat[8 * k + 2 * j + 1]];
        }
    }
    uint8_t rows[64];
    const int ss = g.ss[c], pw = g.plane_w[c];
    if (!ke_idct_scaled<int[64], IdctMul24>(blk, ss, rows, 8) && status[img] == KE_JPEG_OK) status[img] = KE_JPEG_UNSUPPORTED;
    uint8_t *dst = planes + d.plane_off[c] + (size_t)(brow * ss) * pw + bcol * ss;
    if (ss == 8) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            uint2 v;
            v.x = rows[8 * r] | (rows[8 * r + 1] << 8) | (rows[8 * r + 2] << 16) | ((uint32_t)rows[8 * r + 3] << 24);
            v.y = rows[8 * r + 4] | (rows[8 * r + 5] << 8) | (rows[8 * r + 6] << 16) | ((uint32_t)rows[8 * r + 7] << 24);
            *reinterpret_cast<uint2 *>(dst + (size_t)r * pw) = v;
        }
    } else {
        for (int r = 0; r < ss; ++r)
            for (int x = 0; x < ss; ++x) dst[(size_t)r * pw + x] = rows[8 * r + x];
    }
}

// one thread per 4 pixels of a row, as ke_jpeg_colour; the samples are read one by one (planes of a reduced component are as
// narrow as one byte per block, so nothing here may assume a dword inside a row)
__global__ __launch_bounds__(256) void ke_jpeg_colour_scaled(const KeJpegDev *__restrict__ imgs, const KeJpegScaled *__restrict__ geo, int64_t n_imgs,
                                                             int xblocks, const uint8_t *__restrict__ planes, uint8_t *__restrict__ out) {
    const int64_t img = (int64_t)blockIdx.z * 65535 + blockIdx.y;
    if (img >= n_imgs) return;
    const KeJpegDev &d = imgs[img];
    const KeJpegScaled &g = geo[img];
    const int ncomp = d.info.ncomp;
    const int r = threadIdx.x >> 6, q = threadIdx.x & 63;
    const int block_x = (int)(blockIdx.x % (unsigned)xblocks), block_y = (int)(blockIdx.x / (unsigned)xblocks);
    const int x0 = block_x * 256 + q * 4;
    if (x0 >= g.out_w) return;
    const uint8_t *Y = planes + d.plane_off[0], *Cb = planes + d.plane_off[1], *Cr = planes + d.plane_off[2];
    uint8_t *dst = out + d.out_off;
    const int npx = min(4, g.out_w - x0);
    for (int turn = 0; turn < kColourRows / 4; ++turn) {
        const int y = block_y * kColourRows + turn * 4 + r;
        if (y >= g.out_h) break;
        for (int k = 0; k < npx; ++k) {
            const int x = x0 + k;
            const int luma = Y[(size_t)y * g.plane_w[0] + x];
            if (ncomp == 1) {
                dst[(size_t)y * g.out_w + x] = (uint8_t)luma;
                continue;
            }
            const int cb = ke_upsample_scaled_at(Cb, g.plane_w[1], g.comp_w[1], g.comp_h[1], g.hfac[1], g.vfac[1], g.fancy, x, y);
            const int cr = ke_upsample_scaled_at(Cr, g.plane_w[2], g.comp_w[2], g.comp_h[2], g.hfac[2], g.vfac[2], g.fancy, x, y);
            ke_ycc_to_rgb(luma, cb, cr, dst + ((size_t)y * g.out_w + x) * 3);
        }
    }
}

}  // namespace

// (not ke_probe_each: the parser interns Huffman tables, and a pool lives as long as one thread's range of one call)
KE_API int ke_jpeg_probe(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *widths,
                         int32_t *heights, int32_t *channels, int32_t *status_out) {
    if (n < 0 || (n > 0 && (!files || !offsets || !sizes || !widths || !heights || !channels || !status_out))) return KE_EINVAL;
    ke_parallel_ranges(n, [=](int64_t lo, int64_t hi, int) {
        KeJpegTables tables;
        for (int64_t i = lo; i < hi; ++i) {
            KeJpegInfo info;
            ke_parse_jpeg(files + offsets[i], (size_t)sizes[i], tables, info, false);     // headers only
            widths[i] = info.width; heights[i] = info.height; channels[i] = info.ncomp;
            status_out[i] = info.status;
            if (tables.pool.size() > 64) { tables.pool.clear(); tables.keys.clear(); }
        }
    });
    return KE_OK;
}

// EXIF orientation of a JPEG as ImageOps.exif_transpose reads it (tag 0x0112 of IFD0 in the first APP1 "Exif" segment): 1 when
// there is none, -1 when the segment cannot be followed
static int jpeg_orientation(const uint8_t *p, size_t size) {
    size_t pos = 2;
    int found = 1, exif_segments = 0;
    while (pos + 4 <= size && p[pos] == 0xFF) {
        const int m = p[pos + 1];
        if (m == 0xDA || m == 0xD9) break;
        if (m == 0xFF) { ++pos; continue; }
        if ((m >= 0xD0 && m <= 0xD8) || m == 0x01) { pos += 2; continue; }
        const size_t len = ((size_t)p[pos + 2] << 8) | p[pos + 3];
        if (len < 2 || pos + 2 + len > size) return -1;
        if (m == 0xE1 && len >= 8 && std::memcmp(p + pos + 4, "Exif\0\0", 6) == 0) {
            if (++exif_segments > 1) return -1;                   // Pillow strings several segments together
            const uint8_t *t = p + pos + 10;
            const size_t tl = len - 8;
            if (tl < 8) return -1;
            const bool le = t[0] == 'I' && t[1] == 'I', be = t[0] == 'M' && t[1] == 'M';
            if (!le && !be) return -1;
            auto rd16 = [&](size_t o) -> uint32_t { return le ? (uint32_t)(t[o] | (t[o + 1] << 8)) : (uint32_t)((t[o] << 8) | t[o + 1]); };
            auto rd32 = [&](size_t o) -> uint32_t { return le ? rd16(o) | (rd16(o + 2) << 16) : (rd16(o) << 16) | rd16(o + 2); };
            if (rd16(2) != 42) return -1;
            const size_t ifd = rd32(4);
            if (ifd + 2 > tl) return -1;
            const uint32_t entries = rd16(ifd);
            if (ifd + 2 + 12 * (size_t)entries > tl) return -1;
            for (uint32_t e = 0; e < entries; ++e) {
                const size_t o = ifd + 2 + 12 * (size_t)e;
                if (rd16(o) != 0x0112) continue;
                const uint32_t type = rd16(o + 2);
                if (rd32(o + 4) != 1 || (type != 3 && type != 4)) return -1;
                found = (int)(type == 3 ? rd16(o + 8) : rd32(o + 8));
            }
        }
        pos += 2 + len;
    }
    return found;
}

KE_API int ke_jpeg_caveats(const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n, int32_t *flags_out) {
    return ke_caveats_each(files, offsets, sizes, n, flags_out, [](const uint8_t *file, size_t size) {
        const int o = size >= 4 ? jpeg_orientation(file, size) : 1;
        // bits 8..11: the orientation itself where the tag could be followed (1..8), for callers that apply it on the device
        return ((o < 0 || (o >= 2 && o <= 8)) ? KE_CAVEAT_ORIENTATION : 0) | (o >= 1 && o <= 8 ? o << 8 : 0);
    });
}

// ---- the decode call in steps: the switches, prepare (parse, merge, order, gather, geometry) and, per sub-batch of
// ke_decode_sub_batches, the record layout (take), the restart-lane plan, the entropy stage and the pixel stage (launch)

struct JpegSwitches {                  // the environment, read once per call; and KE_TRACE's clock
    bool trace = std::getenv("KE_TRACE") != nullptr;
    bool device_end = !std::getenv("KE_JPEG_HOST_END");              // 1: walk every file's entropy data on the host, as before
    bool keep_order = std::getenv("KE_JPEG_KEEP_ORDER") != nullptr;
    // KE_JPEG_SPLIT_RESTARTS=1: sequential files with restart intervals are decoded interval-wise (ke_jpeg_restarts.h);
    // KE_JPEG_SPLIT_MIN_MCUS: the MCUs a lane should at least have (tuning, and the tests' way to lanes in tiny files)
    bool split = false;
    uint32_t split_min_mcus = KE_RST_MIN_MCUS;
    std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
    JpegSwitches() {
        const char *e = std::getenv("KE_JPEG_SPLIT_RESTARTS");
        split = e && *e && std::strcmp(e, "0") != 0;
        const long v = (e = std::getenv("KE_JPEG_SPLIT_MIN_MCUS")) ? std::atol(e) : 0;
        if (v >= 1) split_min_mcus = (uint32_t)std::min<long>(v, 1l << 30);
    }
    void lap(const char *what) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[ke_jpeg_decode] %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    }
};

// What prepare makes of the caller's files, and the call's device arrays.  Copies are queued from tables.pool, scans and geo:
// a call declares its JpegBatch (and its JpegSubBatch) before its KeStreamGuard.
struct JpegBatch {
    struct Key { uint64_t a, b; uint32_t i; };
    std::vector<Key> order;            // the accepted files in device order: order[k].i is the caller's index
    KeJpegDev *devs = nullptr;         // their records in that order, page-locked (ctx->h_meta)
    KeJpegTables tables;               // one pool for the batch: every part's tables interned again
    std::vector<KeJpegScan> scans;     // of the progressive files, image after image
    std::vector<KeJpegScaled> geo;     // with denoms: the reduced geometry, in device order as devs
    void *d_files = nullptr, *d_tables = nullptr, *d_scans = nullptr;
};

// ctx->h_meta, grown to hold `count` records.
static int jpeg_page_locked_records(ke_ctx *ctx, size_t count, KeJpegDev **devs) {
    const size_t bytes = count * sizeof(KeJpegDev);
    if (ctx->h_meta_bytes < bytes) {
        if (ctx->h_meta) (void)hipHostFree(ctx->h_meta);
        ctx->h_meta = nullptr, ctx->h_meta_bytes = 0;
        KE_HIP(ctx, hipHostMalloc(&ctx->h_meta, bytes + bytes / 4, hipHostMallocDefault));
        ctx->h_meta_bytes = bytes + bytes / 4;
    }
    *devs = (KeJpegDev *)ctx->h_meta;
    return KE_OK;
}

// host: headers, Huffman tables, geometry -- on the host's threads (a header costs a few microseconds; 65 536 of them on one
// thread are more than the kernels take).  A record is 700 bytes (three quantisation tables), so records are written once,
// where they are parsed, and move once more: in device order into the page-locked block they are uploaded from.  (Before:
// per-thread vectors merged into one, copied again by the sort, uploaded from pageable memory -- 50 ms of a 65 536-file call,
// as long as the entropy kernel.)  status_out[i] is the parser's; b.order stays empty when it accepts no file.
static int jpeg_prepare(ke_ctx *ctx, JpegSwitches &sw, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                        const int32_t *denoms, const uint64_t *out_offsets, int32_t *status_out, JpegBatch &b) {
    struct Part {
        KeJpegTables tables;
        std::vector<KeJpegScan> scans;
        int64_t first = 0, last = 0;
        std::vector<int> remap;        // its table numbers -> the batch's
        uint32_t scan_base = 0;        // its first scan among the batch's
    };
    std::unique_ptr<KeJpegDev[]> all(new KeJpegDev[(size_t)n]);           // record i <-> file i; status != OK = not decodable
    std::vector<Part> parts(16);
    const int nparts = ke_parallel_ranges(n, [&](int64_t first, int64_t last, int t) {
        Part &p = parts[(size_t)t];
        p.first = first; p.last = last;
        p.tables.sequential_only = true;
        for (int64_t i = first; i < last; ++i) {
            KeJpegDev &d = all[(size_t)i];
            bool defer = false;
            ke_parse_jpeg(files + offsets[i], (size_t)sizes[i], p.tables, d.info, true, &p.scans, sw.device_end ? &defer : nullptr);
            status_out[i] = d.info.status;
            if (d.info.status != KE_JPEG_OK) continue;
            d.end_on_device = defer ? 1 : 0;
            d.file_size = (uint32_t)sizes[i];
            d.file_off = offsets[i];
            d.out_off = out_offsets[i];
        }
    });
    sw.lap("parse (threads)");
    for (int t = 0; t < nparts; ++t) {
        Part &p = parts[(size_t)t];
        p.scan_base = (uint32_t)b.scans.size();
        b.scans.insert(b.scans.end(), p.scans.begin(), p.scans.end());
        for (const std::vector<uint8_t> &key : p.tables.keys) p.remap.push_back(b.tables.intern(key.data(), key.data() + 16, (int)key.size() - 16));
    }
    // The 64 lanes of a wave step through their images block by block and finish together at best: neighbours in the device
    // order should be images of like geometry and like compressed size (like amounts of work per block).  The order is a sort
    // of (key, file) pairs; the records themselves are gathered afterwards.
    using Key = JpegBatch::Key;
    b.order.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const KeJpegDev &d = all[(size_t)i];
        if (d.info.status != KE_JPEG_OK) continue;
        const KeJpegInfo &in = d.info;
        const uint64_t work = (uint64_t)in.mcus_x * in.mcus_y * in.ncomp, bytes = (d.end_on_device ? d.file_size : in.scan_end) - in.scan_offset;
        b.order.push_back(sw.keep_order ? Key{0, 0, (uint32_t)i} : Key{((uint64_t)(in.progressive ? 1 : 0) << 63) | (~work & 0x7FFFFFFFFFFFFFFFull), ~bytes, (uint32_t)i});
    }
    if (b.order.empty()) return KE_OK;
    if (!sw.keep_order)
        std::sort(b.order.begin(), b.order.end(), [](const Key &x, const Key &y) { return x.a != y.a ? x.a < y.a : x.b != y.b ? x.b < y.b : x.i < y.i; });
    sw.lap("merge tables + order");
    const int64_t total = (int64_t)b.order.size();
    KE_TRY(jpeg_page_locked_records(ctx, (size_t)total, &b.devs));
    auto part_index = [&](int64_t i) { int t = 0; while (t + 1 < nparts && i >= parts[(size_t)t].last) ++t; return t; };
    ke_parallel_ranges(total, [&](int64_t first, int64_t last, int) {
        for (int64_t k = first; k < last; ++k) {
            const int64_t i = b.order[(size_t)k].i;
            KeJpegDev &d = b.devs[k];
            d = all[(size_t)i];
            const Part &p = parts[(size_t)part_index(i)];
            if (d.info.progressive) {
                d.info.first_scan += p.scan_base;
            } else {
                for (int c = 0; c < d.info.ncomp; ++c) {
                    d.info.huff_dc[c] = p.remap[(size_t)d.info.huff_dc[c]];
                    d.info.huff_ac[c] = p.remap[(size_t)d.info.huff_ac[c]];
                }
            }
        }
    });
    if (denoms) {
        b.geo.resize((size_t)total);
        for (int64_t k = 0; k < total; ++k) ke_jpeg_scaled_geometry(b.devs[k].info, denoms[b.order[(size_t)k].i], b.geo[(size_t)k]);
    }
    sw.lap("records into device order");
    return KE_OK;
}

// A sub-batch: what take lays out, and what launch reserves and works off.  Copies are queued from prog_list and rst_files.
struct JpegSubBatch {
    size_t first = 0;                  // its first image in the device order
    uint64_t coef_units = 0, plane_bytes = 0;
    int max_blocks = 0, max_w = 0, max_h = 0, progressive = 0;
    std::vector<int32_t> prog_list;    // its progressive files
    std::vector<KeRstFile> rst_files;  // the files whose restart intervals go to lanes of their own, and the lanes of them all
    uint64_t rst_lanes = 0;
    void *d_imgs = nullptr, *d_coef = nullptr, *d_planes = nullptr;
    int32_t *d_status = nullptr, *d_split = nullptr;     // KE_BUF_OUT0: m status words; behind them m split flags where files are split
    KeRstFile *d_rfiles = nullptr;                       // KE_BUF_TILE32: [records | marker table]
    uint32_t *d_marks = nullptr;
};

// Image k's record laid out in the sub-batch's scratch: coefficients (2 B per sample) + planes (1 B per sample).  One thread
// per image: the larger the sub-batch the better the chip is filled (65 536 images are one wave per SIMD).
static bool jpeg_take(JpegBatch &b, JpegSubBatch &sub, uint64_t lo, uint64_t budget, size_t k, bool fresh) {
    if (fresh) {
        sub.first = k;
        sub.coef_units = sub.plane_bytes = 0;
        sub.max_blocks = sub.max_w = sub.max_h = sub.progressive = 0;
    }
    KeJpegDev &d = b.devs[k];
    // the image index is a pair of grid dimensions (65 535 x 65 535).  Progressive files: at most two waves of them per CU in one
    // launch (measured: a third wave per CU slows all three by more than it adds -- 65 536 files 458 ms in one launch, 417 in two)
    if (k - sub.first >= (1u << 20) || (d.info.progressive && sub.progressive >= 32768)) return false;
    uint64_t blocks = 0, pl = 0;
    for (int c = 0; c < d.info.ncomp; ++c) {
        blocks += (uint64_t)(d.info.plane_w[c] >> 3) * (d.info.plane_h[c] >> 3);
        pl += (uint64_t)d.info.plane_w[c] * d.info.plane_h[c];
    }
    if (!fresh && (sub.coef_units + blocks * 64) * 2 + sub.plane_bytes + pl > budget) return false;
    sub.progressive += d.info.progressive ? 1 : 0;
    d.file_off -= lo;
    d.coef_off = sub.coef_units;
    uint64_t at = 0;
    for (int c = 0; c < 3; ++c) {
        d.block_base[c] = (int32_t)at;
        d.plane_off[c] = sub.plane_bytes;
        if (c < d.info.ncomp) {
            at += (uint64_t)(d.info.plane_w[c] >> 3) * (d.info.plane_h[c] >> 3);
            sub.plane_bytes += ((uint64_t)d.info.plane_w[c] * d.info.plane_h[c] + 15) & ~15ull;
        }
    }
    d.blocks_total = (int32_t)blocks;
    sub.coef_units += blocks * 64;
    sub.max_blocks = std::max(sub.max_blocks, (int)blocks);
    sub.max_w = std::max(sub.max_w, b.geo.empty() ? d.info.width : b.geo[k].out_w);
    sub.max_h = std::max(sub.max_h, b.geo.empty() ? d.info.height : b.geo[k].out_h);
    return true;
}

// The restart-lane plan of a sub-batch: the files whose plan has two lanes or more, with the prefix of their lanes.
static uint64_t jpeg_restart_lanes(const KeJpegDev *devs, int64_t m, uint32_t min_mcus, std::vector<KeRstFile> &rst_files) {
    uint64_t rst_lanes = 0;
    for (int64_t k = 0; k < m; ++k) {
        const KeJpegInfo &in = devs[k].info;
        if (in.progressive || in.restart_interval <= 0) continue;
        const KeRstPlan plan = ke_rst_plan((uint32_t)in.mcus_x * (uint32_t)in.mcus_y, (uint32_t)in.restart_interval, min_mcus, KE_RST_LANE_CAP);
        if (!ke_rst_plan_splits(plan) || rst_lanes + plan.n_lanes > (1ull << 31)) continue;     // (lane indices stay below 2^31)
        rst_files.push_back(KeRstFile{(uint32_t)k, (uint32_t)rst_lanes, plan});
        rst_lanes += plan.n_lanes;
    }
    return rst_lanes;
}

// images per wave: 64 once that makes two waves for every SIMD, fewer (down to 8) below that (measured: 65 536 files 90.1 ms
// at 64 per wave, 86.4 at 32, 103 at 16; 16 384 files 38.3 at 16, 34.5 at 8)
static int jpeg_lanes_for(int64_t images, int64_t waves_wanted) {
    int lanes = 64;
    while (lanes > 8 && (images + lanes / 2 - 1) / (lanes / 2) <= waves_wanted) lanes /= 2;
    return lanes;
}

// The entropy stage of a sub-batch of m images (devs: its records on the host): the ends of the entropy-coded segments, the
// restart markers of the files to split, the one-lane walk, the restart lanes, the progressive files.
static int jpeg_enqueue_entropy(ke_ctx *ctx, JpegSwitches &sw, const JpegBatch &b, JpegSubBatch &s, const KeJpegDev *devs, int64_t m) {
    const KeJpegDev *d_imgs = (const KeJpegDev *)s.d_imgs;
    const uint8_t *d_files = (const uint8_t *)b.d_files;
    const int64_t nrf = (int64_t)s.rst_files.size(), rst_lanes = (int64_t)s.rst_lanes, waves = (int64_t)ctx->cu_count * 8;
    hipLaunchKernelGGL(ke_jpeg_find_end, dim3((unsigned)m), dim3(64), 0, ctx->stream, (KeJpegDev *)s.d_imgs, m, d_files, s.d_status);
    if (nrf) {
        KE_HIP(ctx, hipMemcpyAsync(s.d_rfiles, s.rst_files.data(), (size_t)nrf * sizeof(KeRstFile), hipMemcpyHostToDevice, ctx->stream));
        KE_HIP(ctx, hipMemsetAsync(s.d_split, 0, (size_t)m * 4, ctx->stream));
        hipLaunchKernelGGL(ke_jpeg_find_restarts, dim3((unsigned)nrf), dim3(64), 0, ctx->stream, (KeJpegDev *)s.d_imgs, (const KeRstFile *)s.d_rfiles, nrf,
                           d_files, (const int32_t *)s.d_status, s.d_marks, s.d_split);
        sw.lap("find restarts (enqueue)");
    }
    // sequential files: no clearing of the coefficient array, every block of an image that decodes is written whole (a
    // damaged image's remaining blocks hold whatever was there, and its pixels are discarded with its status);
    // progressive files build their coefficients up scan by scan, from zero
    s.prog_list.clear();
    for (int64_t k = 0; k < m; ++k)
        if (devs[k].info.progressive) s.prog_list.push_back((int32_t)k);
    const int64_t np = (int64_t)s.prog_list.size();
    if (np < m) {
        const int lanes = jpeg_lanes_for(m, waves);
        hipLaunchKernelGGL(ke_jpeg_entropy, dim3((unsigned)((m + lanes - 1) / lanes)), dim3(64), 0, ctx->stream, d_imgs, m, d_files,
                           (const KeHuffTable *)b.d_tables, (int16_t *)s.d_coef, s.d_status, lanes);
    }
    if (nrf) {
        const int lanes = jpeg_lanes_for(rst_lanes, waves);
        hipLaunchKernelGGL(ke_jpeg_entropy_rst, dim3((unsigned)((rst_lanes + lanes - 1) / lanes)), dim3(64), 0, ctx->stream, d_imgs,
                           (const KeRstFile *)s.d_rfiles, nrf, rst_lanes, d_files, (const KeHuffTable *)b.d_tables, (int16_t *)s.d_coef, s.d_status, lanes,
                           (const uint32_t *)s.d_marks, (const int32_t *)s.d_split);
        sw.lap("restart lanes (enqueue)");
    }
    if (np) {
        void *d_list;
        KE_TRY(ke_reserve(ctx, KE_BUF_OUT1, (size_t)np * 4, &d_list));
        KE_HIP(ctx, hipMemcpyAsync(d_list, s.prog_list.data(), (size_t)np * 4, hipMemcpyHostToDevice, ctx->stream));
        for (size_t run0 = 0, run1; run0 < (size_t)np; run0 = run1 + 1) {      // their coefficients to zero, one memset per run of neighbours in the batch
            for (run1 = run0; run1 + 1 < (size_t)np && s.prog_list[run1 + 1] == s.prog_list[run1] + 1;) ++run1;
            const KeJpegDev &from = devs[s.prog_list[run0]], &to = devs[s.prog_list[run1]];
            const uint64_t units = to.coef_off + (uint64_t)to.blocks_total * 64 - from.coef_off;
            KE_HIP(ctx, hipMemsetAsync((int16_t *)s.d_coef + from.coef_off, 0, (size_t)units * 2, ctx->stream));
        }
        const int lanes = jpeg_lanes_for(np, (int64_t)ctx->cu_count * 2);      // two waves of these per CU (see jpeg_take)
        hipLaunchKernelGGL(ke_jpeg_entropy_prog, dim3((unsigned)((np + lanes - 1) / lanes)), dim3(64), 0, ctx->stream, d_imgs, (const int32_t *)d_list, np,
                           d_files, (const KeJpegScan *)b.d_scans, (int16_t *)s.d_coef, s.d_status, lanes);
    }
    return KE_OK;
}

// The pixel stage: IDCT into the planes, then upsampling and colour into the caller's buffer -- at the files' own sizes, or
// (geo: the sub-batch's reduced geometry) at the scaled ones.
static int jpeg_enqueue_pixels(ke_ctx *ctx, const JpegSubBatch &s, int64_t m, const KeJpegScaled *geo, uint8_t *pixels_out) {
    const KeJpegDev *d_imgs = (const KeJpegDev *)s.d_imgs;
    const dim3 idct((unsigned)((s.max_blocks + 255) / 256), (unsigned)std::min<int64_t>(m, 65535), (unsigned)((m + 65534) / 65535));
    const int xblocks = (s.max_w + 255) / 256, yblocks = (s.max_h + kColourRows - 1) / kColourRows;
    const dim3 colour((unsigned)(xblocks * yblocks), idct.y, idct.z);
    if (!geo) {
        hipLaunchKernelGGL(ke_jpeg_idct, idct, dim3(256), 0, ctx->stream, d_imgs, m, (const int16_t *)s.d_coef, (uint8_t *)s.d_planes, s.d_status);
        hipLaunchKernelGGL(ke_jpeg_colour, colour, dim3(256), 0, ctx->stream, d_imgs, m, xblocks, (const uint8_t *)s.d_planes, pixels_out);
        return KE_OK;
    }
    void *d_geo;
    KE_TRY(ke_reserve(ctx, KE_BUF_OUT2, (size_t)m * sizeof(KeJpegScaled), &d_geo));
    KE_HIP(ctx, hipMemcpyAsync(d_geo, geo, (size_t)m * sizeof(KeJpegScaled), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(ke_jpeg_idct_scaled, idct, dim3(256), 0, ctx->stream, d_imgs, (const KeJpegScaled *)d_geo, m, (const int16_t *)s.d_coef,
                       (uint8_t *)s.d_planes, s.d_status);
    hipLaunchKernelGGL(ke_jpeg_colour_scaled, colour, dim3(256), 0, ctx->stream, d_imgs, (const KeJpegScaled *)d_geo, m, xblocks,
                       (const uint8_t *)s.d_planes, pixels_out);
    return KE_OK;
}

// The sub-batch that take packed: its plan, the reserves, the records' copy and the two stages.  Names m status words, or 2 m
// with the split flags behind them.  No file with a plan of two lanes or more: nothing new is reserved or launched.
static int jpeg_launch(ke_ctx *ctx, JpegSwitches &sw, const JpegBatch &b, JpegSubBatch &s, int64_t m, uint8_t *pixels_out, const int32_t **status,
                       size_t *words) {
    const KeJpegDev *devs = b.devs + s.first;
    s.rst_files.clear();
    s.rst_lanes = sw.split ? jpeg_restart_lanes(devs, m, sw.split_min_mcus, s.rst_files) : 0;
    const bool split = !s.rst_files.empty();
    KE_TRY(ke_reserve(ctx, KE_BUF_META, (size_t)m * sizeof(KeJpegDev), &s.d_imgs));
    KE_TRY(ke_reserve(ctx, KE_BUF_TMP, (size_t)s.coef_units * 2 + 64, &s.d_coef));
    KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_IN, (size_t)s.plane_bytes + 64, &s.d_planes));
    KE_TRY(ke_reserve(ctx, KE_BUF_OUT0, (size_t)m * (split ? 8 : 4), (void **)&s.d_status));
    s.d_split = split ? s.d_status + m : nullptr;
    if (split) {
        const size_t rec_bytes = (s.rst_files.size() * sizeof(KeRstFile) + 15) & ~(size_t)15;
        KE_TRY(ke_reserve(ctx, KE_BUF_TILE32, rec_bytes + (size_t)s.rst_lanes * 4, (void **)&s.d_rfiles));
        s.d_marks = (uint32_t *)((uint8_t *)s.d_rfiles + rec_bytes);
    }
    sw.lap("layout + reserve");
    KE_HIP(ctx, hipMemcpyAsync(s.d_imgs, devs, (size_t)m * sizeof(KeJpegDev), hipMemcpyHostToDevice, ctx->stream));
    KE_TRY(jpeg_enqueue_entropy(ctx, sw, b, s, devs, m));
    KE_TRY(jpeg_enqueue_pixels(ctx, s, m, b.geo.empty() ? nullptr : b.geo.data() + s.first, pixels_out));
    *status = s.d_status;
    *words = (size_t)m * (split ? 2 : 1);
    sw.lap("enqueue");
    return KE_OK;
}

// The decode call.  denoms = NULL: ke_jpeg_decode, exactly as before.  Otherwise file i is decoded at 1 / denoms[i]
// (ke_jpeg_decode_scaled): the same parse, order, entropy kernels and scratch, the IDCT and colour kernels of the reduced sizes.
static int jpeg_decode_batch(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                             const int32_t *denoms, uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out) {
    KE_TRY(ke_decode_check_args(ctx, files, offsets, sizes, n, pixels_out, out_offsets, status_out, "compressed files are parsed"));
    ctx->jpeg_files_split = ctx->jpeg_split_lanes = 0;
    if (n == 0) return KE_OK;
    JpegSwitches sw;
    // the compressed bytes set off for the device before anything is parsed: one contiguous range of the caller's buffer (the
    // files the decoder will turn down travel along -- they are the few), 17 ms for the 970 MB of 65 536 files, hidden behind
    // the parsing
    uint64_t lo = ~0ull, hi = 0;
    for (int64_t i = 0; i < n; ++i)
        if (sizes[i]) { lo = std::min(lo, offsets[i]); hi = std::max(hi, offsets[i] + sizes[i]); }
    if (hi <= lo) {
        for (int64_t i = 0; i < n; ++i) status_out[i] = KE_JPEG_CORRUPT;
        return KE_OK;
    }
    JpegBatch batch;
    JpegSubBatch sub;
    KeStreamGuard guard;                                          // after the host vectors it waits for
    KE_TRY(ke_upload_files(ctx, guard, files, lo, hi, KE_BUF_PIXELS, 256, &batch.d_files));   // the stream windows read up to 64 bytes past a file
    KE_TRY(jpeg_prepare(ctx, sw, files, offsets, sizes, n, denoms, out_offsets, status_out, batch));
    if (batch.order.empty()) return KE_OK;                     // (the guard waits: the caller's buffer is still being read)
    KE_TRY(ke_reserve(ctx, KE_BUF_JPEG_TABLES, batch.tables.pool.size() * sizeof(KeHuffTable), &batch.d_tables));
    KE_HIP(ctx, hipMemcpyAsync(batch.d_tables, batch.tables.pool.data(), batch.tables.pool.size() * sizeof(KeHuffTable), hipMemcpyHostToDevice, ctx->stream));
    if (!batch.scans.empty()) {
        KE_TRY(ke_reserve(ctx, KE_BUF_SSIM_AUX, batch.scans.size() * sizeof(KeJpegScan), &batch.d_scans));
        KE_HIP(ctx, hipMemcpyAsync(batch.d_scans, batch.scans.data(), batch.scans.size() * sizeof(KeJpegScan), hipMemcpyHostToDevice, ctx->stream));
    }
    // half of what this context's scratch and the free HBM come to together (a sum that does not move when the scratch is
    // regrown, so that consecutive calls cut their batches alike and keep their buffers), up to 160 GB
    uint64_t budget;
    KE_TRY(ke_scratch_budget(ctx, {KE_BUF_TMP, KE_BUF_SSIM_IN}, (uint64_t)2 << 30, (uint64_t)160 << 30, "KE_JPEG_SCRATCH_BYTES", KE_BUDGET_ENV_LOWERS, &budget));
    KE_TRY(ke_decode_sub_batches(
        ctx, batch.order.size(), [&](size_t k, bool fresh) { return jpeg_take(batch, sub, lo, budget, k, fresh); },
        [&](size_t m, const int32_t **status, size_t *words) { return jpeg_launch(ctx, sw, batch, sub, (int64_t)m, pixels_out, status, words); },
        [&](size_t at, size_t k, size_t m, const int32_t *st) {
            if (k == 0) sw.lap("wait for the stream");
            status_out[batch.order[at].i] = st[k];
            if (k + 1 == m)                                    // the sub-batch's last: what of its plan the device took
                for (const KeRstFile &rf : sub.rst_files)
                    if (st[m + rf.img]) { ++ctx->jpeg_files_split; ctx->jpeg_split_lanes += rf.plan.n_lanes; }
        }));
    guard.disarm();
    return KE_OK;
}

KE_API int ke_jpeg_decode(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                          uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out) {
    return jpeg_decode_batch(ctx, files, offsets, sizes, n, nullptr, pixels_out, out_offsets, status_out);
}

KE_API int ke_jpeg_decode_scaled(ke_ctx *ctx, const uint8_t *files, const uint64_t *offsets, const uint64_t *sizes, int64_t n,
                                 const int32_t *denoms, uint8_t *pixels_out, const uint64_t *out_offsets, int32_t *status_out) {
    if (!ctx) return KE_EINVAL;
    if (n > 0 && !denoms) return ke_fail(ctx, KE_EINVAL, "NULL argument");
    for (int64_t i = 0; i < n; ++i)
        if (denoms[i] != 1 && denoms[i] != 2 && denoms[i] != 4 && denoms[i] != 8)
            return ke_fail(ctx, KE_EINVAL, "file %lld: scale 1/%d (1, 2, 4 or 8)", (long long)i, denoms[i]);
    if (n == 0) denoms = nullptr;
    return jpeg_decode_batch(ctx, files, offsets, sizes, n, denoms, pixels_out, out_offsets, status_out);
}

KE_API int ke_jpeg_last_split(ke_ctx *ctx, int64_t *files_split, int64_t *lanes) {
    if (!ctx) return KE_EINVAL;
    if (files_split) *files_split = ctx->jpeg_files_split;
    if (lanes) *lanes = ctx->jpeg_split_lanes;
    return KE_OK;
}
