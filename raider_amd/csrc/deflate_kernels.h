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
//   deflate_encode_dyn_kernel  the same steps, but every sub-block comes out as the smallest of a stored, a fixed-Huffman and a
//                              dynamic-Huffman block: the steps write tokens to a scratch of the workgroup's own and count their symbols,
//                              optimal length-limited codes are built from the counts, and only the winner is emitted ("dynamic tables").
//   deflate_pack_kernel        one workgroup per sub-block: 78 01 in front of a stream's first sub-block, the slot's bytes or a stored
//                              block (header + input), the big-endian Adler-32 behind the last one.
//   h5_chunks_kernel           a C-ordered array cut into full-size chunks (edges padded with the fill value), each optionally
//                              byte-transposed as HDF5's shuffle filter does.
//
// Determinism: the hash table is updated with atomicMax on positions, the bit window with atomicOr and the symbol counts with
// atomicAdd - all commute, so no byte depends on the order in which they land.  Every loop is bounded by the sub-block length.
//
// deflate_subblock() and deflate_subblock_dyn() are compiled by the host checks too (tools/probes/deflate_host_check.cpp,
// deflate_dynamic_host_check.cpp), with 64 threads standing in for the lanes: the wave operations they use are the wv_* functions
// below and nothing else.
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
DEFL_DEV void wv_atomic_add(uint32_t* p, uint32_t v) { atomicAdd(p, v); }
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

// The length symbol (257 .. 285) of len 3 .. 258 and the distance symbol (0 .. 29) of dist 1 .. 32768, with their extra bits.
DEFL_DEV int defl_len_sym(int len, int& eb, uint32_t& ev) {
    const uint32_t l = (uint32_t)(len - 3);
    eb = 0; ev = 0u;
    if (len == 258) return 285;
    if (l < 8) return 257 + (int)l;
    eb = defl_log2(l) - 2; ev = l & ((1u << eb) - 1u);
    return 261 + 4 * eb + (int)((l >> eb) & 3u);
}

DEFL_DEV int defl_dist_sym(int dist, int& deb, uint32_t& dev) {
    const uint32_t d = (uint32_t)(dist - 1);
    deb = 0; dev = 0u;
    if (d < 4) return (int)d;
    deb = defl_log2(d) - 1; dev = d & ((1u << deb) - 1u);
    return 2 * deb + 2 + (int)((d >> deb) & 1u);
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

// ---- dynamic tables ------------------------------------------------------------------------------------------------------------------
// deflate_subblock_dyn() tokenises once - the matcher's steps, unchanged - into a token scratch in global memory (one per resident
// workgroup) while it counts the literal / length and the distance symbols in LDS.  The counts give the exact size of the fixed and of
// the dynamic block before a bit is written; the smallest of stored, fixed and dynamic is emitted (ties in that order).  No LDS is
// added: the counts live in the bit window while it is idle, and everything after the last step - counts, code lengths, code tables,
// the run-length coded header, the package-merge lists - lies over the hash table, which only the matcher needs.
constexpr int DEFL_NLL = 286, DEFL_ND = 30, DEFL_NCL = 19;
constexpr int DEFL_MAXSYM = 288;                                  // room of an alphabet's arrays
constexpr int DEFL_HIST_D = 288;                                  // the distance counts' place in the window (the literal / length counts start at 0)
// places in S.hash (words) once tokenising has ended
constexpr int DT_CNT_LL = 0, DT_CNT_D = 288, DT_CNT_CL = 320;     // counts
constexpr int DT_LEN_LL = 340, DT_LEN_D = 628, DT_LEN_CL = 660;   // code lengths
constexpr int DT_TAB_LL = 680, DT_TAB_D = 968, DT_TAB_CL = 1000;  // codes as stream bits | length << 16
constexpr int DT_RLE = 1020;                                      // the header's code-length symbols | extra bits << 8, at most 316
constexpr int DT_VARS = 1340;                                     // hlit, hdist, nrle, hclen, header bits
constexpr int DT_WORK = 1348;                                     // defl_build_lengths' work space
constexpr int DEFL_PM_LIST = 2 * DEFL_MAXSYM, DEFL_PM_BMW = DEFL_PM_LIST / 32;     // a package-merge list; the words of its leaf bitmap
constexpr int DEFL_PM_WORK = 2 * DEFL_MAXSYM + 2 * DEFL_PM_LIST + 16 * DEFL_PM_BMW + 16 + 32;
static_assert(DT_WORK + DEFL_PM_WORK <= DEFL_HASH, "the dynamic-table work space must fit over the hash table");
static_assert(DEFL_HIST_D + 32 <= DEFL_WIN_WORDS, "the counts must fit into the bit window");

DEFL_DEV uint32_t wv_sum(int lane, uint32_t v) {                  // the wave's sum of v, in every lane
    for (int d = 1; d < 64; d <<= 1) { const uint32_t u = wv_shfl_up(lane, v, d); if (lane >= d) v += u; }
    return wv_shfl(lane, v, 63);
}

DEFL_DEV int defl_ll_extra(int sym) { return (sym < 265 || sym == 285) ? 0 : (sym - 261) >> 2; }
DEFL_DEV int defl_d_extra(int sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }
DEFL_DEV int defl_fixed_len(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }

// Code lengths of `nsym` <= 286 symbols with counts cnt[], none longer than `limit` <= 15 (2^limit >= nsym), with the smallest
// sum of count * length any such prefix code has: package-merge (Larmore & Hirschberg 1990).  The leaves are ranked by (count, symbol);
// list l is the merge of the leaves with the pairs ("packages") of list l - 1, leaves first among equals; the first 2m - 2 items of list
// `limit` are taken, and a leaf's length is the number of lists it was taken from.  Each list keeps only its weights and one bit per
// item (leaf or package): of the t items taken from list l, the k leaves are the k lightest, the t - k packages take 2 (t - k) items of
// list l - 1.  An alphabet with fewer than two used symbols gets two codes of one bit, as zlib does, so that the code is complete.
// cnt, lens and W (DEFL_PM_WORK words) are LDS (host: plain memory); every lane calls this with the same arguments.
DEFL_DEV void defl_build_lengths(int lane, const uint32_t* cnt, int nsym, int limit, uint32_t* lens, uint32_t* W) {
    uint32_t* sw = W;                                             // the leaves' counts, ascending
    uint32_t* ss = W + DEFL_MAXSYM;                               // their symbols
    uint32_t* la = W + 2 * DEFL_MAXSYM;                           // list l - 1
    uint32_t* lb = la + DEFL_PM_LIST;                             // list l
    uint32_t* bm = lb + DEFL_PM_LIST;                             // [16][DEFL_PM_BMW]: bit i of list l set: item i is a leaf
    uint32_t* kk = bm + 16 * DEFL_PM_BMW;                         // [16]: leaves taken from list l
    int m = 0;
    for (int b = 0; b < nsym; b += 64) m += __builtin_popcountll(wv_ballot(lane, b + lane < nsym && cnt[b + lane] > 0u));
    for (int i = lane; i < nsym; i += 64) lens[i] = 0u;
    wv_sync();
    if (m < 2) {
        if (lane == 0) {
            int u = 0;
            while (u < nsym && cnt[u] == 0u) ++u;
            if (u >= nsym) u = 0;
            lens[u] = 1u; lens[u == 0 ? 1 : 0] = 1u;
        }
        wv_sync();
        return;
    }
    for (int i = lane; i < nsym; i += 64) {
        const uint32_t c = cnt[i];
        if (c == 0u) continue;
        int r = 0;
        for (int j = 0; j < nsym; ++j) { const uint32_t o = cnt[j]; r += (o > 0u && (o < c || (o == c && j < i))) ? 1 : 0; }
        sw[r] = c; ss[r] = (uint32_t)i;
    }
    for (int k = lane; k < 16 * DEFL_PM_BMW + 16; k += 64) bm[k] = 0u;           // (kk follows bm)
    wv_sync();
    const int L = limit < m - 1 ? limit : m - 1;                  // no optimal code of m symbols is deeper than m - 1
    for (int i = lane; i < m; i += 64) la[i] = sw[i];
    int na = m;
    wv_sync();
    for (int l = 2; l <= L; ++l) {
        const int np = na >> 1;
        uint32_t* B = bm + l * DEFL_PM_BMW;
        for (int i = lane; i < m; i += 64) {                      // a leaf goes behind the packages lighter than itself
            const uint32_t w = sw[i];
            int lo = 0, hi = np;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (la[2 * mid] + la[2 * mid + 1] < w) lo = mid + 1; else hi = mid; }
            const int pos = i + lo;
            lb[pos] = w;
            wv_atomic_or(&B[pos >> 5], 1u << (pos & 31));
        }
        for (int j = lane; j < np; j += 64) {                     // a package goes behind the leaves that are not heavier
            const uint32_t w = la[2 * j] + la[2 * j + 1];
            int lo = 0, hi = m;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (sw[mid] <= w) lo = mid + 1; else hi = mid; }
            lb[j + lo] = w;
        }
        wv_sync();
        uint32_t* t = la; la = lb; lb = t;
        na = m + np;
    }
    if (lane == 0) {
        int t = 2 * m - 2;
        for (int l = L; l >= 2; --l) {
            const uint32_t* B = bm + l * DEFL_PM_BMW;
            int k = 0;
            for (int w = 0; w < DEFL_PM_BMW && 32 * w < t; ++w) {
                const int r = t - 32 * w;
                k += __builtin_popcount(r >= 32 ? B[w] : B[w] & ((1u << r) - 1u));
            }
            kk[l] = (uint32_t)k;
            t = 2 * (t - k);
        }
        kk[1] = (uint32_t)(t < m ? t : m);
    }
    wv_sync();
    for (int i = lane; i < m; i += 64) {
        uint32_t n = 0u;
        for (int l = 1; l <= L; ++l) n += kk[l] > (uint32_t)i ? 1u : 0u;
        lens[ss[i]] = n;
    }
    wv_sync();
}

// Canonical codes (RFC 1951 3.2.2) of lens[0 .. nsym) as stream bits | length << 16 into tab[]; W: 32 words of work space.
DEFL_DEV void defl_canonical(int lane, const uint32_t* lens, int nsym, uint32_t* tab, uint32_t* W) {
    if (lane < 32) W[lane] = 0u;
    wv_sync();
    for (int i = lane; i < nsym; i += 64) if (lens[i] > 0u) wv_atomic_add(&W[lens[i]], 1u);
    wv_sync();
    if (lane == 0) {
        uint32_t code = 0u, prev = 0u;
        for (int b = 1; b <= 15; ++b) { code = (code + prev) << 1; prev = W[b]; W[16 + b] = code; }
    }
    wv_sync();
    for (int i = lane; i < nsym; i += 64) {
        const uint32_t n = lens[i];
        uint32_t c = 0u;
        for (int j = 0; j < i; ++j) c += lens[j] == n ? 1u : 0u;
        tab[i] = n > 0u ? (defl_rev(W[16 + n] + c, (int)n) | (n << 16)) : 0u;
    }
    wv_sync();
}

// Every lane's two bit strings (v1 first; nb1 + nb2 <= 48, each <= 32) into the window in lane order; flushes with room for the next call.
DEFL_DEV void defl_emit(int lane, DeflShared& S, uint32_t* slot, uint32_t slot_words, uint32_t& bitpos, uint32_t& wbase, uint32_t v1, int nb1,
                        uint32_t v2, int nb2) {
    const uint32_t nb = (uint32_t)(nb1 + nb2);
    uint32_t off = nb;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t u = wv_shfl_up(lane, off, d); if (lane >= d) off += u; }
    const uint32_t total = wv_shfl(lane, off, 63);
    const uint32_t at = bitpos - 32u * wbase + off - nb;
    defl_put(S.win, at, v1, nb1);
    defl_put(S.win, at + (uint32_t)nb1, v2, nb2);
    bitpos += total;
    wv_sync();
    // a call adds at most 64 * 48 bits = 96 words: flushed 32 words early, the window's DEFL_STEP_WORDS of slack hold them
    if (bitpos - 32u * wbase >= 32u * (uint32_t)(DEFL_WIN_WORDS - 32)) wbase = defl_flush(lane, S, slot, slot_words, wbase, bitpos, false);
}

// What follows the last step in the dynamic mode: S.win holds the counts, tok[0 .. ntok) the tokens (a literal byte, or
// bit 31 | (len - 3) << 15 | (dist - 1)).  The smallest of a stored, a fixed-Huffman and a dynamic-Huffman block is written.
// R.fixed_bytes: the bytes in the slot (0: stored); R.pad: 2 when they are a dynamic block.
DEFL_DEV DeflResult defl_finish_dyn(int lane, DeflShared& S, int n, bool last, uint32_t* __restrict__ slot, const uint32_t* __restrict__ tok, int ntok, DeflResult R) {
    const uint32_t* hist = S.win;
    // ---- the counts move over the hash table; the three sizes
    uint32_t* T = S.hash;
    for (int k = lane; k < DT_WORK; k += 64) T[k] = 0u;
    wv_sync();
    uint32_t fixed_bits = 0u, extra_bits = 0u;
    for (int s = lane; s < DEFL_NLL; s += 64) {
        const uint32_t c = hist[s] + (s == 256 ? 1u : 0u);                            // the end-of-block symbol
        T[DT_CNT_LL + s] = c;
        fixed_bits += c * (uint32_t)defl_fixed_len(s); extra_bits += c * (uint32_t)defl_ll_extra(s);
    }
    if (lane < DEFL_ND) {
        const uint32_t c = hist[DEFL_HIST_D + lane];
        T[DT_CNT_D + lane] = c;
        fixed_bits += c * 5u; extra_bits += c * (uint32_t)defl_d_extra(lane);
    }
    wv_sync();
    extra_bits = wv_sum(lane, extra_bits);
    fixed_bits = 3u + wv_sum(lane, fixed_bits) + extra_bits;
    defl_build_lengths(lane, T + DT_CNT_LL, DEFL_NLL, 15, T + DT_LEN_LL, T + DT_WORK);
    defl_build_lengths(lane, T + DT_CNT_D, DEFL_ND, 15, T + DT_LEN_D, T + DT_WORK);
    const uint8_t order[DEFL_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    if (lane == 0) {                                                                  // HLIT, HDIST, the lengths run-length coded, their counts
        int nl = DEFL_NLL, nd = DEFL_ND;
        while (nl > 257 && T[DT_LEN_LL + nl - 1] == 0u) --nl;
        while (nd > 1 && T[DT_LEN_D + nd - 1] == 0u) --nd;
        const int N = nl + nd;
        int i = 0, nr = 0;
        while (i < N) {
            const uint32_t v = i < nl ? T[DT_LEN_LL + i] : T[DT_LEN_D + i - nl];
            int run = 1;
            while (i + run < N && (i + run < nl ? T[DT_LEN_LL + i + run] : T[DT_LEN_D + i + run - nl]) == v) ++run;
            i += run;
            if (v != 0u) { T[DT_RLE + nr++] = v; T[DT_CNT_CL + v] += 1u; --run; }
            while (run > 0) {
                uint32_t sym, ex; int take;
                if (v == 0u && run >= 11) { take = run < 138 ? run : 138; sym = 18u; ex = (uint32_t)(take - 11); }
                else if (v == 0u && run >= 3) { take = run; sym = 17u; ex = (uint32_t)(take - 3); }
                else if (v != 0u && run >= 3) { take = run < 6 ? run : 6; sym = 16u; ex = (uint32_t)(take - 3); }
                else { take = 1; sym = v; ex = 0u; }
                T[DT_RLE + nr++] = sym | (ex << 8); T[DT_CNT_CL + sym] += 1u;
                run -= take;
            }
        }
        T[DT_VARS + 0] = (uint32_t)nl; T[DT_VARS + 1] = (uint32_t)nd; T[DT_VARS + 2] = (uint32_t)nr;
    }
    wv_sync();
    defl_build_lengths(lane, T + DT_CNT_CL, DEFL_NCL, 7, T + DT_LEN_CL, T + DT_WORK);
    if (lane == 0) {
        int hclen = DEFL_NCL;
        while (hclen > 4 && T[DT_LEN_CL + order[hclen - 1]] == 0u) --hclen;
        uint32_t hb = 3u + 14u + 3u * (uint32_t)hclen + 2u * T[DT_CNT_CL + 16] + 3u * T[DT_CNT_CL + 17] + 7u * T[DT_CNT_CL + 18];
        for (int s = 0; s < DEFL_NCL; ++s) hb += T[DT_CNT_CL + s] * T[DT_LEN_CL + s];
        T[DT_VARS + 3] = (uint32_t)hclen; T[DT_VARS + 4] = hb;
    }
    wv_sync();
    uint32_t dyn_bits = 0u;
    for (int s = lane; s < DEFL_NLL; s += 64) dyn_bits += T[DT_CNT_LL + s] * T[DT_LEN_LL + s];
    if (lane < DEFL_ND) dyn_bits += T[DT_CNT_D + lane] * T[DT_LEN_D + lane];
    dyn_bits = T[DT_VARS + 4] + wv_sum(lane, dyn_bits) + extra_bits;
    // a block's bytes: its bits (the end-of-block code among them), the empty stored block's 3, zeros to the byte boundary, 00 00 FF FF
    const uint32_t stored_bytes = (uint32_t)n + 5u;
    const uint32_t fixed_bytes = (fixed_bits + 3u + 7u) / 8u + 4u, dyn_bytes = (dyn_bits + 3u + 7u) / 8u + 4u;
    const bool dyn = dyn_bytes < stored_bytes && dyn_bytes < fixed_bytes;
    if (!dyn && fixed_bytes >= stored_bytes) return R;                                // stored: the pack kernel copies the input
    // ---- the code tables, the header
    const uint32_t slot_words = (uint32_t)DEFL_SLOT / 4u;
    for (int k = lane; k < DEFL_WIN_WORDS + DEFL_STEP_WORDS + 4; k += 64) S.win[k] = 0u;
    if (dyn) {
        defl_canonical(lane, T + DT_LEN_LL, DEFL_NLL, T + DT_TAB_LL, T + DT_WORK);
        defl_canonical(lane, T + DT_LEN_D, DEFL_ND, T + DT_TAB_D, T + DT_WORK);
        defl_canonical(lane, T + DT_LEN_CL, DEFL_NCL, T + DT_TAB_CL, T + DT_WORK);
    } else {
        for (int s = lane; s < DEFL_NLL; s += 64) { int nb; const uint32_t v = defl_fixed_sym(s, nb); T[DT_TAB_LL + s] = v | ((uint32_t)nb << 16); }
        if (lane < DEFL_ND) T[DT_TAB_D + lane] = defl_rev((uint32_t)lane, 5) | (5u << 16);
        wv_sync();
    }
    uint32_t bitpos = 3u, wbase = 0u;
    if (lane == 0) defl_put(S.win, 0u, dyn ? 4u : 2u, 3);                              // BFINAL 0, BTYPE 10 or 01
    if (dyn) {
        const int nl = (int)T[DT_VARS + 0], nd = (int)T[DT_VARS + 1], nr = (int)T[DT_VARS + 2], hclen = (int)T[DT_VARS + 3];
        if (lane == 0) defl_put(S.win, 3u, (uint32_t)(nl - 257) | ((uint32_t)(nd - 1) << 5) | ((uint32_t)(hclen - 4) << 10), 14);
        if (lane < hclen) defl_put(S.win, 17u + 3u * (uint32_t)lane, T[DT_LEN_CL + order[lane]], 3);
        bitpos = 17u + 3u * (uint32_t)hclen;
        wv_sync();
        for (int b = 0; b < nr; b += 64) {
            uint32_t v1 = 0u, v2 = 0u; int nb1 = 0, nb2 = 0;
            if (b + lane < nr) {
                const uint32_t r = T[DT_RLE + b + lane], sym = r & 0xffu, c = T[DT_TAB_CL + sym];
                v1 = c & 0xffffu; nb1 = (int)(c >> 16);
                v2 = r >> 8; nb2 = sym == 16u ? 2 : sym == 17u ? 3 : sym == 18u ? 7 : 0;
            }
            defl_emit(lane, S, slot, slot_words, bitpos, wbase, v1, nb1, v2, nb2);
        }
    } else wv_sync();
    // ---- the tokens
    for (int b = 0; b < ntok; b += 64) {
        uint32_t v1 = 0u, v2 = 0u; int nb1 = 0, nb2 = 0;
        if (b + lane < ntok) {
            const uint32_t t = tok[b + lane];
            if (t & 0x80000000u) {
                int eb, deb; uint32_t ev, dev;
                const uint32_t c = T[DT_TAB_LL + defl_len_sym((int)((t >> 15) & 0xffu) + 3, eb, ev)];
                const uint32_t d = T[DT_TAB_D + defl_dist_sym((int)(t & 0x7fffu) + 1, deb, dev)];
                nb1 = (int)(c >> 16); v1 = (c & 0xffffu) | (ev << nb1); nb1 += eb;
                nb2 = (int)(d >> 16); v2 = (d & 0xffffu) | (dev << nb2); nb2 += deb;
            } else {
                const uint32_t c = T[DT_TAB_LL + t];
                v1 = c & 0xffffu; nb1 = (int)(c >> 16);
            }
        }
        defl_emit(lane, S, slot, slot_words, bitpos, wbase, v1, nb1, v2, nb2);
    }
    // ---- end of block, the empty stored block: BFINAL | 00, zeros to the byte boundary, 00 00 FF FF
    {
        const uint32_t c = T[DT_TAB_LL + 256];
        const uint32_t nb = c >> 16;
        if (lane == 0) defl_put(S.win, bitpos - 32u * wbase, c & 0xffffu, (int)nb);
        if (lane == 0 && last) defl_put(S.win, bitpos + nb - 32u * wbase, 1u, 1);
        bitpos += nb + 3u;
        bitpos = (bitpos + 7u) & ~7u;
        if (lane == 0) defl_put(S.win, bitpos + 16u - 32u * wbase, 0xFFFFu, 16);
        bitpos += 32u;
        wv_sync();
        (void)defl_flush(lane, S, slot, slot_words, wbase, bitpos, true);
        R.fixed_bytes = (int32_t)(bitpos / 8u);                                       // (= dyn_bytes or fixed_bytes, below n + 5 <= DEFL_SLOT)
        R.pad = dyn ? 2 : 0;
    }
    return R;
}

// One sub-block: src[0 .. n) -> slot (DEFL_SLOT bytes, 4-byte aligned).  `last`: BFINAL goes on the closing empty stored block.
// Every lane of the wave calls this with the same arguments; lane 0's result is written by the caller.
// DYN: the steps write tokens to tok (DEFL_SUB words of this workgroup's own) and count their symbols in place of emitting bits, and
// defl_finish_dyn() writes the block; without it the function is the fixed-table encoder, statement for statement.
template <bool DYN>
DEFL_DEV DeflResult deflate_subblock_t(int lane, DeflShared& S, const uint8_t* __restrict__ src, int n, bool last, uint32_t* __restrict__ slot,
                                       uint32_t* __restrict__ tok) {
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
    if constexpr (!DYN) {
        if (lane == 0) defl_put(S.win, 0u, 2u, 3);                                    // BFINAL 0, BTYPE 01
        wv_sync();
    }
    int ntok = 0;                                                                     // (DYN)
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
        if constexpr (DYN) {                                                          // the window is idle: the counts live there
            const bool emit = p < n && !covered;
            const uint64_t E = wv_ballot(lane, emit);
            if (emit) {
                uint32_t t;
                if (len > 0) {
                    int eb, deb; uint32_t ev, dev;
                    wv_atomic_add(&S.win[defl_len_sym(len, eb, ev)], 1u);
                    wv_atomic_add(&S.win[DEFL_HIST_D + defl_dist_sym(dist, deb, dev)], 1u);
                    t = 0x80000000u | ((uint32_t)(len - 3) << 15) | (uint32_t)(dist - 1);
                } else {
                    t = in[p];
                    wv_atomic_add(&S.win[t], 1u);
                }
                tok[ntok + __builtin_popcountll(E & ((1ull << lane) - 1ull))] = t;  // (ntok + rank < n: a token covers a byte or more)
            }
            ntok += __builtin_popcountll(E);
            base += cur;
            wv_sync();
            continue;
        }
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
    if constexpr (DYN) return defl_finish_dyn(lane, S, n, last, slot, tok, ntok, R);
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

DEFL_DEV DeflResult deflate_subblock(int lane, DeflShared& S, const uint8_t* __restrict__ src, int n, bool last, uint32_t* __restrict__ slot) {
    return deflate_subblock_t<false>(lane, S, src, n, last, slot, nullptr);
}

// One sub-block as the smallest of a stored, a fixed-Huffman and a dynamic-Huffman block over the tokens of the same steps.
DEFL_DEV DeflResult deflate_subblock_dyn(int lane, DeflShared& S, const uint8_t* __restrict__ src, int n, bool last, uint32_t* __restrict__ slot,
                                         uint32_t* __restrict__ tok) {
    return deflate_subblock_t<true>(lane, S, src, n, last, slot, tok);
}

#if defined(__HIPCC__) && !defined(RDR_DEFLATE_HOST_EMU)

// The dynamic-table mode: as deflate_encode_kernel, with workgroup b's token scratch at tok + b * DEFL_SUB.
__global__ __launch_bounds__(64) void deflate_encode_dyn_kernel(const uint8_t* __restrict__ src, const DeflSub* __restrict__ subs, int64_t nsub,
                                                               uint8_t* __restrict__ slots, DeflResult* __restrict__ res, uint32_t* __restrict__ tok) {
    __shared__ __attribute__((aligned(16))) DeflShared S;
    const int lane = threadIdx.x;
    for (int64_t s = blockIdx.x; s < nsub; s += gridDim.x) {
        const DeflSub d = subs[s];
        const DeflResult r = deflate_subblock_dyn(lane, S, src + d.src_off, d.n, (d.flags & 2) != 0, reinterpret_cast<uint32_t*>(slots + s * (int64_t)DEFL_SLOT),
                                                  tok + (int64_t)blockIdx.x * DEFL_SUB);
        if (lane == 0) res[s] = r;
        __syncthreads();
    }
}

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

// an array cut into chunks: what h5_chunks_kernel and its inverse (h5_unchunk_kernel, inflate_kernels.h) both walk
struct H5ChunkGrid {
    int64_t shape[4], chunk[4], nchunk[4];         // padded to four axes with ones in front
    int64_t chunk_elems, total_elems;              // elements of one chunk; of all chunks the kernel walks
};

struct H5ChunkLayout : H5ChunkGrid {
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
