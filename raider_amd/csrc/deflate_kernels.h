// deflate_kernels.h - zlib streams written on the device, and the chunk cutter that feeds them.
//
//   deflate_encode_kernel      one wave (= one workgroup of 64 lanes) per SUB-BLOCK of DEFL_SUB input bytes.  The sub-block is staged in
//                              LDS, its Adler-32 sums are taken, and it is encoded as ONE fixed-Huffman block followed by an empty stored
//                              block (the Z_SYNC_FLUSH construction: the output ends on a byte boundary and can be moved by a byte copy).
//                              64 positions per step: every lane hashes the three bytes at its position, looks ONE candidate up in a hash
//                              table in LDS (plus distances 1, 2, 4 and 8, which the table cannot hold inside a step), measures the match,
//                              and the wave picks a greedy non-overlapping set from the ballot of the lanes that found one.  A match runs
//                              on past the step, up to 258 bytes.  Token bit lengths are prefix-summed and the codes OR-ed into an LDS bit
//                              window that is flushed in whole words to the sub-block's slot.  A sub-block that would not come out
//                              smaller than a stored block is abandoned: the pack kernel then copies its input.
//   deflate_pack_kernel        one workgroup per sub-block: 78 01 in front of a stream's first sub-block, the slot's bytes or a stored
//                              block (header + input), the big-endian Adler-32 behind the last one.
//   h5_chunks_kernel           a C-ordered array cut into full-size chunks (edges padded with the fill value), each optionally
//                              byte-transposed as HDF5's shuffle filter does.
//
// Determinism: the hash table is updated with atomicMax on positions and the bit window with atomicOr - both commute, so no byte
// depends on the order in which they land.  Every loop is bounded by the sub-block length.
//
// deflate_subblock() is compiled by the host check too (tools/probes/deflate_host_check.cpp), with 64 threads standing in for the
// lanes: the wave operations it uses are the wv_* functions below and nothing else.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define DEFL_DEV __device__ __forceinline__
#else
#define DEFL_DEV inline
#endif

namespace rdr {

constexpr int DEFL_SUB = 32768;            // input bytes of a sub-block
constexpr int DEFL_HASH_BITS = 12;
constexpr int DEFL_HASH = 1 << DEFL_HASH_BITS;
constexpr int DEFL_WIN_WORDS = 1024;       // the bit window: 4 KiB
constexpr int DEFL_STEP_WORDS = 64;        // a step adds at most 64 tokens of 31 bits = 62 words
constexpr int DEFL_SLOT = DEFL_SUB + 512;  // bytes of a sub-block's slot: an abandoned block stops within 8 * 31 bytes of n + 5
constexpr int DEFL_MIN_MATCH = 3, DEFL_MAX_MATCH = 258;
constexpr int DEFL_NEAR = 4096;            // a match of 3 bytes is taken only from this near (zlib's TOO_FAR: a far one costs more bits than three literals)

struct DeflSub {                           // one sub-block, filled by the host
    int64_t src_off;                       // its first byte in src
    int64_t dst_off;                       // where its output starts in out (the stream's 78 01 included for a first sub-block)
    int32_t n;                             // input bytes, 1 .. DEFL_SUB
    int32_t flags;                         // 1: first of its stream, 2: last of its stream
    uint32_t adler;                        // the stream's Adler-32 (last sub-block)
    int32_t fixed_bytes;                   // bytes in the slot, 0: stored
};

struct DeflResult { int32_t fixed_bytes; uint32_t s1, s2; int32_t pad; };     // s1 = sum b[i], s2 = sum (n - i) b[i], both mod 65521

struct DeflShared {                        // 32 KiB + 16 KiB + 4 KiB + a few words: three workgroups per compute unit (160 KiB)
    uint8_t in[DEFL_SUB + 8];              // staged at in[a + i], a = the source address mod 4
    uint32_t hash[DEFL_HASH];              // position + 1 of the latest occurrence, 0: none
    uint32_t win[DEFL_WIN_WORDS + DEFL_STEP_WORDS + 4];
};

#if defined(__HIPCC__) && !defined(RDR_DEFLATE_HOST_EMU)
DEFL_DEV void wv_sync() { __syncthreads(); }
DEFL_DEV uint64_t wv_ballot(int lane, bool p) { (void)lane; return __ballot(p); }
DEFL_DEV uint32_t wv_shfl(int lane, uint32_t v, int src) { (void)lane; return (uint32_t)__shfl((int)v, src, 64); }
DEFL_DEV uint32_t wv_shfl_up(int lane, uint32_t v, int d) { (void)lane; return (uint32_t)__shfl_up((int)v, d, 64); }
DEFL_DEV void wv_atomic_max(uint32_t* p, uint32_t v) { atomicMax(p, v); }
DEFL_DEV void wv_atomic_or(uint32_t* p, uint32_t v) { atomicOr(p, v); }
#endif

DEFL_DEV uint32_t defl_rev(uint32_t v, int n) {        // the low n bits of v, reversed (Huffman codes go MSB first into an LSB-first stream)
    v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
    v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
    v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
    v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
    v = (v >> 16) | (v << 16);
    return v >> (32 - n);
}

DEFL_DEV int defl_log2(uint32_t v) { return 31 - __builtin_clz(v); }      // v > 0

// A literal / length symbol of the fixed code (RFC 1951 3.2.6) as stream bits.
DEFL_DEV uint32_t defl_fixed_sym(int sym, int& nbits) {
    if (sym < 144) { nbits = 8; return defl_rev(0x30u + (uint32_t)sym, 8); }
    if (sym < 256) { nbits = 9; return defl_rev(0x190u + (uint32_t)(sym - 144), 9); }
    if (sym < 280) { nbits = 7; return defl_rev((uint32_t)(sym - 256), 7); }
    nbits = 8;
    return defl_rev(0xC0u + (uint32_t)(sym - 280), 8);
}

// A match (len 3 .. 258, dist 1 .. 32768) as stream bits, at most 8 + 5 + 5 + 13 = 31 of them.
DEFL_DEV uint32_t defl_match_bits(int len, int dist, int& nbits) {
    int sym, eb = 0; uint32_t ev = 0;
    const uint32_t l = (uint32_t)(len - 3);
    if (len == 258) sym = 285;
    else if (l < 8) sym = 257 + (int)l;
    else { eb = defl_log2(l) - 2; sym = 261 + 4 * eb + (int)((l >> eb) & 3u); ev = l & ((1u << eb) - 1u); }
    int nb;
    uint32_t v = defl_fixed_sym(sym, nb);
    v |= ev << nb; nb += eb;
    const uint32_t d = (uint32_t)(dist - 1);
    int dsym, deb = 0; uint32_t dev = 0;
    if (d < 4) dsym = (int)d;
    else { deb = defl_log2(d) - 1; dsym = 2 * deb + 2 + (int)((d >> deb) & 1u); dev = d & ((1u << deb) - 1u); }
    v |= defl_rev((uint32_t)dsym, 5) << nb; nb += 5;
    v |= dev << nb; nb += deb;
    nbits = nb;
    return v;
}

// `nbits` <= 32 bits of v into the window at bit `at` (window-relative; at + nbits <= 32 * (DEFL_WIN_WORDS + DEFL_STEP_WORDS)).
DEFL_DEV void defl_put(uint32_t* win, uint32_t at, uint32_t v, int nbits) {
    if (nbits <= 0) return;
    const uint32_t w = at >> 5, s = at & 31u;
    wv_atomic_or(&win[w], v << s);
    if (s + (uint32_t)nbits > 32u) wv_atomic_or(&win[w + 1], v >> (32u - s));
}

// Whole words of the window -> the slot, the rest moved to the front.  `bitpos` counts from the sub-block's first output bit; the
// window starts at word `wbase` of the slot.  Words at or beyond slot_words are dropped (an abandoned block).  Returns the new wbase.
DEFL_DEV uint32_t defl_flush(int lane, DeflShared& S, uint32_t* slot, uint32_t slot_words, uint32_t wbase, uint32_t bitpos, bool all) {
    const uint32_t rel = bitpos - 32u * wbase;
    const uint32_t full = all ? (rel + 31u) >> 5 : rel >> 5;                        // words to write
    for (uint32_t k = (uint32_t)lane; k < full; k += 64u)
        if (wbase + k < slot_words) slot[wbase + k] = S.win[k];
    wv_sync();
    const uint32_t keep = all ? 0u : S.win[full];                                   // (full <= DEFL_WIN_WORDS + DEFL_STEP_WORDS)
    wv_sync();
    for (uint32_t k = (uint32_t)lane; k < (uint32_t)(DEFL_WIN_WORDS + DEFL_STEP_WORDS + 4); k += 64u) S.win[k] = (k == 0u) ? keep : 0u;
    wv_sync();
    return wbase + full;
}

// One sub-block: src[0 .. n) -> slot (DEFL_SLOT bytes, 4-byte aligned).  `last`: BFINAL goes on the closing empty stored block.
// Every lane of the wave calls this with the same arguments; lane 0's result is written by the caller.
DEFL_DEV DeflResult deflate_subblock(int lane, DeflShared& S, const uint8_t* __restrict__ src, int n, bool last, uint32_t* __restrict__ slot) {
    DeflResult R{0, 0u, 0u, 0};
    if (n < 1) return R;
    if (n > DEFL_SUB) n = DEFL_SUB;
    // ---- stage: bytes up to a word boundary of the source, whole words, the bytes behind them
    const int a = (int)(reinterpret_cast<uintptr_t>(src) & 3u);
    uint8_t* in = S.in + a;
    {
        const int head = (4 - a) & 3, h = head < n ? head : n;
        const int words = (n - h) >> 2, tail0 = h + 4 * words;
        if (lane < h) in[lane] = src[lane];
        for (int k = lane; k < words; k += 64)
            *reinterpret_cast<uint32_t*>(in + h + 4 * k) = *reinterpret_cast<const uint32_t*>(src + h + 4 * k);
        if (tail0 + lane < n) in[tail0 + lane] = src[tail0 + lane];
        for (int k = lane; k < DEFL_HASH; k += 64) S.hash[k] = 0u;
        for (int k = lane; k < DEFL_WIN_WORDS + DEFL_STEP_WORDS + 4; k += 64) S.win[k] = 0u;
    }
    wv_sync();
    // ---- Adler-32 sums: lane l takes bytes l, l + 64, ...; reduced mod 65521 every 64 bytes (64 * 32768 * 255 < 2^32)
    {
        uint32_t s1 = 0u, s2 = 0u, t2 = 0u; int cnt = 0;
        for (int i = lane; i < n; i += 64) {
            const uint32_t b = in[i];
            s1 += b; t2 += (uint32_t)(n - i) * b;
            if (++cnt == 64) { s2 = (s2 + t2 % 65521u) % 65521u; t2 = 0u; cnt = 0; }
        }
        s2 = (s2 + t2 % 65521u) % 65521u;
        s1 %= 65521u;                                                                 // (512 * 255 per lane: far below 2^32)
        for (int d = 1; d < 64; d <<= 1) {                                            // inclusive scan; lane 63 holds the sums
            const uint32_t u1 = wv_shfl_up(lane, s1, d), u2 = wv_shfl_up(lane, s2, d);
            if (lane >= d) { s1 = (s1 + u1) % 65521u; s2 = (s2 + u2) % 65521u; }
        }
        R.s1 = wv_shfl(lane, s1, 63); R.s2 = wv_shfl(lane, s2, 63);
    }
    // ---- the fixed block
    const uint32_t stored_bytes = (uint32_t)n + 5u;
    const uint32_t slot_words = (uint32_t)DEFL_SLOT / 4u;
    uint32_t bitpos = 3u, wbase = 0u;
    if (lane == 0) defl_put(S.win, 0u, 2u, 3);                                        // BFINAL 0, BTYPE 01
    wv_sync();
    int base = 0;
    bool abandoned = false;
    while (base < n) {                                                                // base grows by at least 64 per turn
        const int p = base + lane;
        const bool canhash = p + DEFL_MIN_MATCH <= n;
        uint32_t cand = 0u, h = 0u;
        uint32_t w = 0u;
        if (canhash) {
            w = (uint32_t)in[p] | ((uint32_t)in[p + 1] << 8) | ((uint32_t)in[p + 2] << 16);
            h = (w * 2654435761u) >> (32 - DEFL_HASH_BITS);
            cand = S.hash[h];
        }
        wv_sync();                                                                    // every lookup sees the table as the last step left it
        if (canhash) wv_atomic_max(&S.hash[h], (uint32_t)p + 1u);
        int len = 0, dist = 0;
        if (canhash) {
            const int maxlen = n - p < DEFL_MAX_MATCH ? n - p : DEFL_MAX_MATCH;
            if (cand > 0u && (int)cand - 1 < p) {
                const int c = (int)cand - 1;
                int k = 0;
                while (k < maxlen && in[c + k] == in[p + k]) ++k;
                if (k > DEFL_MIN_MATCH || (k == DEFL_MIN_MATCH && p - c <= DEFL_NEAR)) { len = k; dist = p - c; }
            }
            // the table holds nothing of this step: distances 1 (runs), 2, 4 and 8 (the periods of 2-, 4- and 8-byte samples) are tried as well
#pragma unroll
            for (int dd = 1; dd <= 8; dd <<= 1) {
                if (p < dd || len >= maxlen) continue;
                const uint32_t u = (uint32_t)in[p - dd] | ((uint32_t)in[p - dd + 1] << 8) | ((uint32_t)in[p - dd + 2] << 16);
                if (u != w) continue;
                int k = DEFL_MIN_MATCH;
                while (k < maxlen && in[p - dd + k] == in[p + k]) ++k;
                if (k > len || (k == len && dd < dist)) { len = k; dist = dd; }
            }
        }
        // greedy choice along the step: the first lane with a match takes it, the lanes it covers emit nothing
        const uint64_t M = wv_ballot(lane, len > 0);
        bool covered = false;
        int cur = 0;
        while (cur < 64) {                                                            // at most 22 turns: a match is 3 bytes or more
            const uint64_t rest = M >> cur;
            if (rest == 0ull) break;
            const int m = cur + __builtin_ctzll(rest);
            const int L = (int)wv_shfl(lane, (uint32_t)len, m);
            if (lane > m && lane < m + L) covered = true;
            cur = m + L;
        }
        if (cur < 64) cur = 64;
        int nb = 0; uint32_t v = 0u;
        if (p < n && !covered) {
            if (len > 0) v = defl_match_bits(len, dist, nb);
            else v = defl_fixed_sym((int)in[p], nb);
        }
        uint32_t off = (uint32_t)nb;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t u = wv_shfl_up(lane, off, d); if (lane >= d) off += u; }
        const uint32_t total = wv_shfl(lane, off, 63);
        defl_put(S.win, bitpos - 32u * wbase + off - (uint32_t)nb, v, nb);
        bitpos += total;
        base += cur;
        wv_sync();
        if ((bitpos + 7u) / 8u + 5u >= stored_bytes) { abandoned = true; break; }     // EOB and the closing block add 5 bytes or more
        if (bitpos - 32u * wbase >= 32u * (uint32_t)DEFL_WIN_WORDS) wbase = defl_flush(lane, S, slot, slot_words, wbase, bitpos, false);
    }
    if (!abandoned) {
        // end of block (7 zero bits), the empty stored block: BFINAL | 00, zeros to the byte boundary, 00 00 FF FF
        if (lane == 0 && last) defl_put(S.win, bitpos + 7u - 32u * wbase, 1u, 1);
        bitpos += 10u;
        bitpos = (bitpos + 7u) & ~7u;
        if (lane == 0) defl_put(S.win, bitpos + 16u - 32u * wbase, 0xFFFFu, 16);
        bitpos += 32u;
        wv_sync();
        const uint32_t bytes = bitpos / 8u;
        if (bytes < stored_bytes && bytes <= (uint32_t)DEFL_SLOT) {
            (void)defl_flush(lane, S, slot, slot_words, wbase, bitpos, true);
            R.fixed_bytes = (int32_t)bytes;
        }
    }
    return R;
}

#if defined(__HIPCC__) && !defined(RDR_DEFLATE_HOST_EMU)

__global__ __launch_bounds__(64) void deflate_encode_kernel(const uint8_t* __restrict__ src, const DeflSub* __restrict__ subs, int64_t nsub,
                                                           uint8_t* __restrict__ slots, DeflResult* __restrict__ res) {
    __shared__ __attribute__((aligned(16))) DeflShared S;
    const int lane = threadIdx.x;
    for (int64_t s = blockIdx.x; s < nsub; s += gridDim.x) {
        const DeflSub d = subs[s];
        const DeflResult r = deflate_subblock(lane, S, src + d.src_off, d.n, (d.flags & 2) != 0, reinterpret_cast<uint32_t*>(slots + s * (int64_t)DEFL_SLOT));
        if (lane == 0) res[s] = r;
        __syncthreads();
    }
}

// out_total: nothing at or beyond it is written, whatever the table says.
__global__ __launch_bounds__(256) void deflate_pack_kernel(const uint8_t* __restrict__ src, const DeflSub* __restrict__ subs, int64_t nsub,
                                                          const uint8_t* __restrict__ slots, uint8_t* __restrict__ out, int64_t out_total) {
    for (int64_t s = blockIdx.x; s < nsub; s += gridDim.x) {
        const DeflSub d = subs[s];
        int64_t o = d.dst_off;
        const int64_t body = d.fixed_bytes > 0 ? (int64_t)d.fixed_bytes : (int64_t)d.n + 5;
        const int64_t end = o + ((d.flags & 1) ? 2 : 0) + body + ((d.flags & 2) ? 4 : 0);
        if (o < 0 || end > out_total || d.n < 1 || d.n > DEFL_SUB) continue;
        if (d.flags & 1) {
            if (threadIdx.x == 0) { out[o] = 0x78; out[o + 1] = 0x01; }
            o += 2;
        }
        if (d.fixed_bytes > 0) {
            const uint8_t* f = slots + s * (int64_t)DEFL_SLOT;
            for (int k = threadIdx.x; k < d.fixed_bytes; k += 256) out[o + k] = f[k];
        } else {
            if (threadIdx.x == 0) {
                out[o] = (d.flags & 2) ? 1 : 0;                                       // BFINAL, BTYPE 00, the byte's other bits unused
                out[o + 1] = (uint8_t)(d.n & 0xff); out[o + 2] = (uint8_t)(d.n >> 8);
                out[o + 3] = (uint8_t)(~d.n & 0xff); out[o + 4] = (uint8_t)((~d.n >> 8) & 0xff);
            }
            const uint8_t* f = src + d.src_off;
            for (int k = threadIdx.x; k < d.n; k += 256) out[o + 5 + k] = f[k];
        }
        o += body;
        if ((d.flags & 2) && threadIdx.x == 0) {
            out[o] = (uint8_t)(d.adler >> 24); out[o + 1] = (uint8_t)(d.adler >> 16); out[o + 2] = (uint8_t)(d.adler >> 8); out[o + 3] = (uint8_t)d.adler;
        }
    }
}

// Horizontal differencing (TIFF predictor 2) of rows of `width` samples of type U, in place of a copy: out[y][x] = in[y][x] - in[y][x-1].
template <typename U>
__global__ __launch_bounds__(256) void tiff_predict_kernel(const U* __restrict__ in, int64_t n, int64_t width, U* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const U v = in[i];
        out[i] = (i % width) ? (U)(v - in[i - 1]) : v;
    }
}

struct H5ChunkLayout {
    int64_t shape[4], chunk[4], nchunk[4];         // padded to four axes with ones in front
    int64_t chunk_elems, total_elems;              // elements of one chunk; of all chunks
    int es, shuffle;
    uint8_t fill[8];
};

__global__ __launch_bounds__(256) void h5_chunks_kernel(const uint8_t* __restrict__ a, H5ChunkLayout L, uint8_t* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < L.total_elems; e += (int64_t)gridDim.x * 256) {
        const int64_t c = e / L.chunk_elems, i = e % L.chunk_elems;
        int64_t ci = c, ii = i, src = 0;
        bool inside = true;
        int64_t idx[4];
        for (int d = 3; d >= 0; --d) {
            const int64_t x = (ci % L.nchunk[d]) * L.chunk[d] + ii % L.chunk[d];
            ci /= L.nchunk[d]; ii /= L.chunk[d];
            idx[d] = x;
            inside = inside && x < L.shape[d];
        }
        if (inside) src = ((idx[0] * L.shape[1] + idx[1]) * L.shape[2] + idx[2]) * L.shape[3] + idx[3];
        uint8_t* o = out + c * L.chunk_elems * L.es;
        for (int j = 0; j < L.es; ++j) {
            const uint8_t b = inside ? a[src * L.es + j] : L.fill[j];
            if (L.shuffle) o[(int64_t)j * L.chunk_elems + i] = b; else o[i * L.es + j] = b;
        }
    }
}

#endif  // __HIPCC__

}  // namespace rdr
