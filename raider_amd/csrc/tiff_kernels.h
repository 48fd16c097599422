// tiff_kernels.h - GeoTIFF segments on the device: TIFF-flavoured LZW decoding and the assembly of decoded tiles / strips into a raster.
//
//   tiff_lzw_kernel            one wave (= one workgroup of 64 lanes) per LZW segment.  The string table lives in LDS (prefix, length,
//                              last byte, first byte: 6 B x 4096 = 24 KB).  Lane 0 reads up to 64 codes and updates the table through
//                              lzw_next() - the one function the host probe (tools/probes/lzw_host_check.cpp) compiles too - then every
//                              lane expands one code: a backward walk of the prefix chain into an LDS staging window, which the wave
//                              flushes with coalesced stores.  The output is NEVER read back: a decoder that copies a string from
//                              where the output already holds it would re-read bytes the same wave has just stored to global memory,
//                              which needs a coherence rule; the table walk needs none.
//   tiff_assemble_kernel<U>    one wave per segment row: clips tile padding, swaps bytes, undoes predictor 2 (a wave scan per 64
//                              samples with a carry between chunks, in the sample's own unsigned type) and writes the band-major raster.
//
// Every index is checked against the segment's input range, its output slot and the table size before it is used: a damaged stream
// ends with a status, never with an access outside its own bytes.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else
#define __host__
#define __device__
#endif

namespace rdr {

enum { LZW_OK = 0, LZW_SHORT = 1, LZW_BAD_CODE = 2 };
enum { LZW_CLEAR = 256, LZW_EOI = 257, LZW_FIRST = 258, LZW_TABLE = 4096 };
enum { LZW_END_EOI = -1, LZW_END_INPUT = -2, LZW_END_BAD = -3,
       LZW_MORE_WINDOW = -4,      // the staged window ran out, the segment has not: restage from s.pos and call again (nothing is lost)
       LZW_CLEARED = -5 };        // a Clear code was taken: entries from 258 up are about to be reused

struct LzwTable {                 // (LDS on the device, plain memory in the host probe); entries 0..255 are the single bytes
    uint16_t* prefix;             // the code this entry extends
    uint16_t* length;             // bytes of its string
    uint8_t* last;                // its last byte
    uint8_t* first;               // its first byte
};

struct LzwState {
    uint32_t pos;                 // next input byte
    uint32_t acc;                 // bits read and not yet used (the low `nacc` bits)
    int nacc;
    int width;                    // current code width, 9..12
    int next;                     // next free table entry
    int prev;                     // the previous data code, -1 right after a Clear
};

__host__ __device__ inline void lzw_reset(LzwState& s) { s.width = 9; s.next = LZW_FIRST; s.prev = -1; }

__host__ __device__ inline void lzw_table_init(const LzwTable& t, int lane, int nlanes) {
    for (int i = lane; i < 256; i += nlanes) { t.prefix[i] = 0; t.length[i] = 1; t.last[i] = (uint8_t)i; t.first[i] = (uint8_t)i; }
}

// The bit reader and the table update: the next DATA code of the stream (its string is then in the table), or a negative LZW_* word.  Input bytes
// are win[p - win_base] for p in [win_base, win_base + win_len) - the caller keeps the window ahead of s.pos - and p < nbytes always.
// TIFF flavour: MSB-first codes, Clear = 256, EOI = 257, the width grows one code early (libtiff's rule: when the next free entry
// reaches 2^width - 1).
__host__ __device__ inline int lzw_next(const uint8_t* win, uint32_t win_base, uint32_t win_len, uint32_t nbytes, LzwState& s, const LzwTable& t) {
    {
        while (s.nacc < s.width) {
            if (s.pos >= nbytes) return LZW_END_INPUT;
            if (s.pos < win_base || s.pos - win_base >= win_len) return LZW_MORE_WINDOW;
            s.acc = (s.acc << 8) | win[s.pos - win_base];
            s.nacc += 8;
            ++s.pos;
        }
        const int code = (int)((s.acc >> (s.nacc - s.width)) & ((1u << s.width) - 1u));
        s.nacc -= s.width;
        s.acc &= (1u << s.nacc) - 1u;
        if (code == LZW_EOI) return LZW_END_EOI;
        if (code == LZW_CLEAR) { lzw_reset(s); return LZW_CLEARED; }
        if (s.prev < 0) {                                   // first code after a Clear: a single byte, nothing to add
            if (code >= 256) return LZW_END_BAD;
            s.prev = code;
            return code;
        }
        if (code > s.next || code >= LZW_TABLE || (code == s.next && s.next >= LZW_TABLE)) return LZW_END_BAD;
        if (s.next < LZW_TABLE) {
            const int n = s.next;
            t.prefix[n] = (uint16_t)s.prev;
            t.length[n] = (uint16_t)(t.length[s.prev] + 1);
            t.first[n] = t.first[s.prev];
            t.last[n] = code == n ? t.first[s.prev] : t.first[code];       // (code == n: the string is prev + its own first byte)
            ++s.next;
            if (s.next >= (1 << s.width) - 1 && s.width < 12) ++s.width;
        }
        s.prev = code;
        return code;
    }
}

// Bytes [from, to) of `code`'s string (positions within the string), written to dst[k - from + dst_off].  Walks the prefix chain from
// the string's end; at most `length` steps, every code read from the table is below LZW_TABLE by construction and checked again.
__host__ __device__ inline void lzw_expand(const LzwTable& t, int code, int from, int to, uint8_t* dst, int dst_off) {
    int k = (int)t.length[code] - 1;
    while (k >= from && code < LZW_TABLE && code >= 0) {
        if (k < to) dst[k - from + dst_off] = t.last[code];
        if (k == 0) break;
        code = t.prefix[code];
        --k;
    }
}

#ifdef __HIPCC__
}  // namespace rdr
#include <type_traits>
namespace rdr {

constexpr int LZW_WINDOW = 4096;        // staged output bytes per flush
constexpr int LZW_INPUT = 128;          // staged input bytes: a batch of 64 codes of 12 bits reads 96 (lzw_next asks for more should it ever need them)

// out slots are at out + i * out_stride; status[i] as LZW_*.  produced bytes never exceed seg_out_bytes[i] (checked on the host
// against out_stride); bytes of a slot the stream does not reach are left as they are.
__global__ __launch_bounds__(64) void tiff_lzw_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ seg_offset,
                                                     const int64_t* __restrict__ seg_bytes, const int64_t* __restrict__ seg_out_bytes, int nseg,
                                                     uint8_t* __restrict__ out, int64_t out_stride, int32_t* __restrict__ status) {
    __shared__ uint16_t s_prefix[LZW_TABLE];
    __shared__ uint16_t s_length[LZW_TABLE];
    __shared__ uint8_t s_last[LZW_TABLE];
    __shared__ uint8_t s_first[LZW_TABLE];
    __shared__ __attribute__((aligned(16))) uint8_t s_stage[LZW_WINDOW + 4];
    __shared__ uint8_t s_in[LZW_INPUT];
    __shared__ int s_code[64];
    __shared__ uint32_t s_off[65];        // output offset of each code of the batch, [ncodes] = the batch's end
    __shared__ int s_ctl[2];              // codes in the batch; how the stream ended (0: it goes on)
    const LzwTable tab{s_prefix, s_length, s_last, s_first};
    const int lane = threadIdx.x;
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        // the segment's input range, clipped to the buffer; its output slot, clipped to the stride
        int64_t so = seg_offset[seg], sb = seg_bytes[seg], cap64 = seg_out_bytes[seg];
        if (so < 0 || so > src_bytes) { so = 0; sb = 0; }
        if (sb < 0) sb = 0;
        if (sb > src_bytes - so) sb = src_bytes - so;
        if (sb > 0x7fffff00LL) sb = 0x7fffff00LL;
        if (cap64 < 0) cap64 = 0;
        if (cap64 > out_stride) cap64 = out_stride;
        if (cap64 > 0x7fffff00LL) cap64 = 0x7fffff00LL;
        const uint8_t* in = src + so;
        const uint32_t nbytes = (uint32_t)sb, cap = (uint32_t)cap64;
        uint8_t* dst = out + (int64_t)seg * out_stride;
        const uint32_t align = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);     // staging index == global address (mod 4)
        lzw_table_init(tab, lane, 64);
        LzwState st{0, 0, 0, 9, LZW_FIRST, -1};        // (lane 0's copy is the one that counts)
        uint32_t produced = 0;
        int result = -1;
        __syncthreads();
        while (result < 0) {
            // stage the next input bytes: whatever lies between st.pos and the segment's end, up to LZW_INPUT
            const uint32_t base = (uint32_t)__shfl((int)st.pos, 0, 64);
            for (int i = lane; i < LZW_INPUT; i += 64) s_in[i] = (base + (uint32_t)i < nbytes) ? in[base + (uint32_t)i] : (uint8_t)0;
            __syncthreads();
            if (lane == 0) {
                int n = 0, end = 0;
                uint32_t o = produced;
                while (n < 64) {
                    const int code = lzw_next(s_in, base, LZW_INPUT, nbytes, st, tab);
                    // a Clear ends the batch: the codes before it are expanded from the entries the codes after it would overwrite
                    if (code == LZW_MORE_WINDOW || code == LZW_CLEARED) break;
                    if (code < 0) { end = code == LZW_END_EOI ? 1 : code == LZW_END_INPUT ? 2 : 3; break; }
                    s_code[n] = code;
                    s_off[n] = o;
                    o += s_length[code];
                    ++n;
                    if (o >= cap) break;
                }
                s_off[n] = o;
                s_ctl[0] = n;
                s_ctl[1] = end;
            }
            __syncthreads();
            const int ncodes = s_ctl[0], end = s_ctl[1];
            const uint32_t batch_end = s_off[ncodes] < cap ? s_off[ncodes] : cap;              // bytes beyond the slot are dropped
            // expand: windows of the virtual position q = align + output offset
            for (uint32_t w0 = (align + produced) / LZW_WINDOW * LZW_WINDOW; w0 < align + batch_end; w0 += LZW_WINDOW) {
                const uint32_t qlo = w0 > align + produced ? w0 : align + produced;
                const uint32_t qhi = w0 + LZW_WINDOW < align + batch_end ? w0 + LZW_WINDOW : align + batch_end;
                if (lane < ncodes) {
                    const int code = s_code[lane];
                    const uint32_t a = align + s_off[lane], b = a + s_length[code];           // the string's range in q
                    const uint32_t lo = a > qlo ? a : qlo, hi = b < qhi ? b : qhi;
                    if (lo < hi) lzw_expand(tab, code, (int)(lo - a), (int)(hi - a), s_stage, (int)(lo - w0));
                }
                __syncthreads();
                // flush q in [qlo, qhi): bytes up to a 4-byte boundary, whole words, bytes behind the last whole word
                const uint32_t wlo = (qlo + 3u) & ~3u, whi = qhi & ~3u;
                if (wlo >= whi) {
                    for (uint32_t q = qlo + lane; q < qhi; q += 64) dst[q - align] = s_stage[q - w0];
                } else {
                    if (qlo + lane < wlo) dst[qlo + lane - align] = s_stage[qlo + lane - w0];
                    for (uint32_t q = wlo + 4u * lane; q < whi; q += 256)
                        *reinterpret_cast<uint32_t*>(dst + (q - align)) = *reinterpret_cast<const uint32_t*>(s_stage + (q - w0));
                    if (whi + lane < qhi) dst[whi + lane - align] = s_stage[whi + lane - w0];
                }
                __syncthreads();
            }
            const bool overflow = s_off[ncodes] > cap;
            produced = batch_end;
            if (overflow) result = LZW_SHORT;                                   // the stream holds more than the slot
            else if (end == 1) result = LZW_OK;
            else if (end == 2) result = produced == cap ? LZW_OK : LZW_SHORT;   // no EOI: fine when the slot is full, as libtiff has it
            else if (end == 3) result = LZW_BAD_CODE;
            __syncthreads();                                                    // (s_ctl / s_off are rewritten by the next batch)
        }
        if (lane == 0) status[seg] = result;
        __syncthreads();
    }
}

// ---- assembly ------------------------------------------------------------------------------------------------------------------
struct TiffLayout {
    int64_t height, width;          // the raster
    int64_t tile_h, tile_w;         // rows / columns of a segment (strips: tile_w == width, tile_h = RowsPerStrip)
    int64_t tiles_x, tiles_y;       // segments across and down one plane
    int64_t seg_stride;             // bytes between decoded segments
    int bands, planar;              // SamplesPerPixel; 1 chunky, 2 planar
    int band;                       // the band to take (0-based), -1: all (band-major output)
    int predictor, swap;
};

template <typename U> __device__ __forceinline__ U tiff_bswap(U v);
template <> __device__ __forceinline__ uint8_t tiff_bswap(uint8_t v) { return v; }
template <> __device__ __forceinline__ uint16_t tiff_bswap(uint16_t v) { return (uint16_t)((v << 8) | (v >> 8)); }
template <> __device__ __forceinline__ uint32_t tiff_bswap(uint32_t v) { return __builtin_bswap32(v); }
template <> __device__ __forceinline__ uint64_t tiff_bswap(uint64_t v) { return __builtin_bswap64(v); }

template <typename A> __device__ __forceinline__ A tiff_shfl_up(A v, int d);
template <> __device__ __forceinline__ uint32_t tiff_shfl_up(uint32_t v, int d) { return (uint32_t)__shfl_up((int)v, d, 64); }
template <> __device__ __forceinline__ uint64_t tiff_shfl_up(uint64_t v, int d) { return (uint64_t)__shfl_up((long long)v, d, 64); }

template <typename A> __device__ __forceinline__ A tiff_lane63(A v);
template <> __device__ __forceinline__ uint32_t tiff_lane63(uint32_t v) { return (uint32_t)__shfl((int)v, 63, 64); }
template <> __device__ __forceinline__ uint64_t tiff_lane63(uint64_t v) { return (uint64_t)__shfl((long long)v, 63, 64); }

// One wave per (plane, segment, row within it); 256 lanes = 4 waves per workgroup.  U: the sample as unsigned bits.
template <typename U>
__global__ __launch_bounds__(256) void tiff_assemble_kernel(const uint8_t* __restrict__ segs, TiffLayout L, U* __restrict__ out) {
    typedef typename std::conditional<(sizeof(U) > 4), uint64_t, uint32_t>::type A;      // the scan's type: wraps like U once truncated
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (int64_t)gridDim.x * 4;
    const int spp = L.planar == 2 ? 1 : L.bands;                  // samples per pixel inside a segment
    const int nplanes = L.planar == 2 ? (L.band < 0 ? L.bands : 1) : 1;
    const int64_t per_plane = L.tiles_x * L.tiles_y;
    const int64_t nrows = (int64_t)nplanes * per_plane * L.tile_h;
    const int c_lo = (L.planar == 2 || L.band < 0) ? 0 : L.band, c_hi = (L.planar == 2) ? 1 : (L.band < 0 ? L.bands : L.band + 1);
    for (int64_t row = wave; row < nrows; row += nwaves) {
        const int64_t r = row % L.tile_h, t = row / L.tile_h;
        const int64_t plane = t / per_plane, ts = t % per_plane, ty = ts / L.tiles_x, tx = ts % L.tiles_x;
        const int64_t y = ty * L.tile_h + r;
        if (y >= L.height) continue;                              // bottom padding / the short last strip
        const int64_t file_plane = L.planar == 2 ? (L.band < 0 ? plane : L.band) : 0;
        const U* in = reinterpret_cast<const U*>(segs + (file_plane * per_plane + ts) * L.seg_stride) + r * L.tile_w * spp;
        const int64_t x0 = tx * L.tile_w;
        const int64_t nx = L.width - x0 < L.tile_w ? L.width - x0 : L.tile_w;             // columns left of the right padding
        for (int c = c_lo; c < c_hi; ++c) {
            const int64_t ob = L.band < 0 ? (L.planar == 2 ? plane : c) : 0;
            U* o = out + (ob * L.height + y) * L.width + x0;
            A carry = 0;
            for (int64_t xb = 0; xb < nx; xb += 64) {
                const int64_t x = xb + lane;
                A v = 0;
                if (x < nx) { U s = in[x * spp + c]; v = (A)(L.swap ? tiff_bswap<U>(s) : s); }
                if (L.predictor == 2) {                            // inclusive scan of the 64 differences, plus what came before
#pragma unroll
                    for (int d = 1; d < 64; d <<= 1) { const A u = tiff_shfl_up<A>(v, d); if (lane >= d) v += u; }
                    v += carry;
                    carry = tiff_lane63<A>(v);                       // (lanes beyond nx added zeros: lane 63 holds the row's sum so far)
                }
                if (x < nx) o[x] = (U)v;
            }
        }
    }
}

#endif  // __HIPCC__

}  // namespace rdr
