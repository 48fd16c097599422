// inflate_kernels.h - zlib streams (RFC 1950 wrapper, RFC 1951 body) decoded on the device, and the inverse of the chunk cutter
// (DESIGN.md 5h).
//
//   inflate_kernel             one wave (= one workgroup of 64 lanes) per stream.  The 32 KiB history is a ring in LDS that doubles as
//                              the output staging area: matches are copied from the ring and the ring is flushed with coalesced stores
//                              (bytes up to a 4-byte boundary of the global address, whole words, bytes), so every output byte is stored
//                              once and none is ever loaded.  Lane 0 decodes a batch of up to 64 tokens through inflate_next() - the
//                              one function the host probe (tools/probes/inflate_host_check.cpp) compiles too - from a 64-bit bit
//                              buffer in registers, refilled a word at a time from a staged input window; a symbol is one read of a
//                              flat table in LDS (10 bits for literal / length, 9 for distance; longer codes take a canonical walk).
//                              The wave then writes the batch into the ring IN TOKEN ORDER: a run of literals by its lanes, a match
//                              cooperatively.  Stored blocks are a cooperative copy from the input.  The Adler-32 is taken from the
//                              ring as it is flushed.
//   h5_unchunk_kernel          decoded HDF5 chunks -> the C-ordered array: edge chunks clipped, the shuffle undone, bytes swapped.
//
// The copy-order rules (ring of exactly 32768 bytes, index = (global address of the byte) mod 32768 up to a multiple of 4):
//   * tokens are applied in stream order, so the byte a token overwrites (32768 positions back) is one no later token may name;
//   * a match with dist < len repeats its own output: byte k is read from start - dist + k mod dist, always a byte from before
//     the match;
//   * a match at distance 32768 - d, d < len, reads ring slots that the same match writes (lane k reads the slot lane k + d
//     writes): every step of 64 bytes reads all its bytes, passes a barrier, and only then writes;
//   * at most 8 KiB + one batch (64 * 258 bytes) are ever unflushed, so a slot is flushed long before it is written again.
//
// status == 0 exactly when zlib's inflate (1.2.11, as zlib.decompress drives it) accepts the stream and its output fits the slot.
// Every index - input byte, table entry, ring byte, output byte - is checked against its range (or masked into it) before use.
#pragma once
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#include "deflate_kernels.h"   // H5ChunkGrid
#define INFL_HD __host__ __device__ inline
#else
#define INFL_HD inline
#endif

namespace rdr {

enum { INFL_OK = 0, INFL_SHORT = 1, INFL_OVERFLOW = 2, INFL_INVALID = 3, INFL_CHECKSUM = 4 };
// what inflate_next() returns besides a token (>= 0)
enum { INFL_EV_DONE = -1,         // the final block ended and the trailer was read: st.adler holds the stream's Adler-32
       INFL_EV_STORED = -2,       // a stored block: st.stored_len bytes follow at st.b.pos (the bit buffer is empty); the caller copies them
                                  // and calls inflate_stored_done()
       INFL_EV_MORE = -3,         // the staged window ran out, the stream has not: restage from st.b.pos and call again (nothing is lost)
       INFL_EV_SHORT = -4,        // the input ended inside the stream
       INFL_EV_INVALID = -5 };
enum { INFL_RING = 32768, INFL_RING_MASK = INFL_RING - 1,
       INFL_WIN = 2048,           // staged input bytes; a dynamic block header reads at most 562 of them, a token 6
       INFL_WIN_LOW = 768,        // restage before a batch when fewer than this many staged bytes are left
       INFL_LBITS = 10, INFL_DBITS = 9, INFL_CBITS = 7,
       INFL_FLUSH = 8192,         // flush the ring once this many bytes wait
       INFL_TOK_MATCH = 1 << 30 };
// a token: a literal 0 .. 255, or INFL_TOK_MATCH | len << 16 | dist (len 3 .. 258, dist 1 .. 32768)
INFL_HD int infl_tok_len(int t) { return (t & INFL_TOK_MATCH) ? ((t >> 16) & 0x1ff) : 1; }
INFL_HD int infl_tok_dist(int t) { return t & 0xffff; }

struct InflCode {                 // one prefix code: a flat table over the next `bits` stream bits, and what the canonical walk needs
    uint16_t* table;              // 1 << bits entries: symbol << 4 | length, 0 = not here (a longer code, or none)
    uint16_t* perm;               // the symbols in order of (length, symbol)
    uint16_t* count;              // [16] codes of each length
    int bits;
};

struct InflShared {               // 32 KiB + 2 KiB + 2 x 3.9 KiB + 1.5 KiB = 43.5 KiB: three workgroups per compute unit (160 KiB)
    uint8_t ring[INFL_RING];
    uint32_t in[INFL_WIN / 4];
    uint16_t fix_lit[1 << INFL_LBITS], fix_dist[1 << INFL_DBITS], dyn_lit[1 << INFL_LBITS], dyn_dist[1 << INFL_DBITS];
    uint16_t fix_lit_perm[288], fix_dist_perm[32], dyn_lit_perm[288], dyn_dist_perm[32];
    uint16_t cl_table[1 << INFL_CBITS], cl_perm[20];
    uint16_t counts[5][16];       // fixed lit, fixed dist, dynamic lit, dynamic dist, code lengths
    uint16_t offs[16];
    uint8_t lens[320];
    int tok[64];
    uint32_t off[65];             // output offset of each token of the batch, [ntok] = the batch's end
    uint32_t ctl[5];              // tokens, event, stored length, input position, Adler-32 read
};

struct InflTables { InflCode fix_lit, fix_dist, dyn_lit, dyn_dist, cl; uint8_t* lens; uint16_t* offs; };

template <typename Shared> INFL_HD InflTables infl_tables(Shared& S) {   // InflShared, or InflMeasureShared (the same tables without the ring)
    return InflTables{InflCode{S.fix_lit, S.fix_lit_perm, S.counts[0], INFL_LBITS}, InflCode{S.fix_dist, S.fix_dist_perm, S.counts[1], INFL_DBITS},
                      InflCode{S.dyn_lit, S.dyn_lit_perm, S.counts[2], INFL_LBITS}, InflCode{S.dyn_dist, S.dyn_dist_perm, S.counts[3], INFL_DBITS},
                      InflCode{S.cl_table, S.cl_perm, S.counts[4], INFL_CBITS}, S.lens, S.offs};
}

// The input as the bit reader sees it.  Positions are VIRTUAL: v = m + p for byte p of the stream, m = the stream's global address mod
// 4, so that v mod 4 == 0 is a word boundary of the staged window (and of global memory).  The window holds v in [base, end).
struct InflIn { const uint8_t* win; uint32_t base, end, nend; };      // nend: the stream's end; end <= nend

struct InflBits { uint32_t pos; uint64_t buf; int n; };               // next byte to load; the low n bits of buf are unread

struct InflState {
    InflBits b;
    int mode;                     // 0: the zlib header is next, 1: a block header, 2: symbols of a fixed block, 3: of a dynamic block, 4: the trailer, 5: done
    int final;                    // the current block is the last
    uint32_t stored_len, adler;
};

INFL_HD void inflate_init(InflState& st, uint32_t m) { st.b.pos = m; st.b.buf = 0; st.b.n = 0; st.mode = 0; st.final = 0; st.stored_len = 0; st.adler = 0; }

INFL_HD uint32_t infl_rev(uint32_t v, int n) {        // the low n bits of v, reversed (1 <= n <= 15)
    v = ((v >> 1) & 0x5555u) | ((v & 0x5555u) << 1);
    v = ((v >> 2) & 0x3333u) | ((v & 0x3333u) << 2);
    v = ((v >> 4) & 0x0f0fu) | ((v & 0x0f0fu) << 4);
    v = ((v >> 8) & 0x00ffu) | ((v & 0x00ffu) << 8);
    return v >> (16 - n);
}

// Bytes into the bit buffer, a word at a time where the position allows it, until more than 32 bits wait or the window / the stream ends.
INFL_HD void infl_refill(const InflIn& in, InflBits& b) {
    while (b.n <= 56) {
        if (b.pos < in.base || b.pos >= in.end) return;
        const uint32_t i = b.pos - in.base;
        if ((b.pos & 3u) == 0u && b.n <= 32 && in.end - b.pos >= 4u) {
            uint32_t w;
#ifdef __HIP_DEVICE_COMPILE__
            w = *reinterpret_cast<const uint32_t*>(in.win + i);
#else
            w = (uint32_t)in.win[i] | (uint32_t)in.win[i + 1] << 8 | (uint32_t)in.win[i + 2] << 16 | (uint32_t)in.win[i + 3] << 24;
#endif
            b.buf |= (uint64_t)w << b.n;
            b.n += 32; b.pos += 4u;
            return;
        }
        b.buf |= (uint64_t)in.win[i] << b.n;
        b.n += 8; ++b.pos;
    }
}

// A refill left the reader short of bits: can another window help?  Yes when the stream goes on behind the window, and when the
// position lies BEFORE it - a stored-block header hands the whole bytes of the bit buffer back, and they may have been loaded from
// the window before this one.
INFL_HD bool infl_more(const InflIn& in, const InflBits& b) { return b.pos < in.base || in.end < in.nend; }

// Make `k` <= 32 bits available: 0, or INFL_EV_MORE / INFL_EV_SHORT.
INFL_HD int infl_need(const InflIn& in, InflBits& b, int k) {
    if (b.n >= k) return 0;
    infl_refill(in, b);
    if (b.n >= k) return 0;
    infl_refill(in, b);                                // (a byte-wise stretch in front of a word boundary)
    if (b.n >= k) return 0;
    return infl_more(in, b) ? INFL_EV_MORE : INFL_EV_SHORT;
}

// The staging rule, shared with the host probe: restage before a batch when nothing is staged yet, when the last batch asked for it,
// when the position lies before the window, or when fewer than INFL_WIN_LOW staged bytes are left and the stream goes on.
INFL_HD bool infl_restage(const InflIn& in, uint32_t vpos, bool first, bool more) {
    return first || more || vpos < in.base || (vpos + (uint32_t)INFL_WIN_LOW > in.end && in.end < in.nend);
}

INFL_HD void infl_window(InflIn& in, uint32_t vpos) {  // the window that starts at the word of vpos
    in.base = vpos & ~3u;
    in.end = in.nend - in.base < (uint32_t)INFL_WIN ? in.nend : in.base + (uint32_t)INFL_WIN;
}

INFL_HD uint32_t infl_take(InflBits& b, int k) {       // k <= 32 bits that infl_need() made available
    const uint32_t v = (uint32_t)(b.buf & ((1ull << k) - 1ull));
    b.buf >>= k; b.n -= k;
    return v;
}

// The code of `n` lengths (lens[s] in 0 .. 15), as zlib 1.2.11's inflate_table decides: 0 built, -1 over-subscribed or incomplete.
// An incomplete set is allowed only as ONE code of length 1, and never for the code-length code (`single_ok`); no codes at all builds
// a table in which every lookup is invalid.  Serial: lane 0 runs it.
INFL_HD int infl_build(const InflCode& c, const uint8_t* lens, int n, bool single_ok, uint16_t* offs) {
    for (int l = 0; l < 16; ++l) c.count[l] = 0;
    for (int s = 0; s < n; ++s) c.count[lens[s] & 15]++;
    const int size = 1 << c.bits;
    for (int k = 0; k < size; ++k) c.table[k] = 0;
    if (c.count[0] == n) return 0;
    int left = 1, max = 0;
    for (int l = 1; l < 16; ++l) {
        left <<= 1;
        left -= c.count[l];
        if (left < 0) return -1;
        if (c.count[l]) max = l;
    }
    if (left > 0 && !(single_ok && max == 1)) return -1;
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + c.count[l]);
    for (int s = 0; s < n; ++s) {
        const int l = lens[s] & 15;
        if (l) c.perm[offs[l]++] = (uint16_t)s;
    }
    uint32_t code = 0; int idx = 0;
    for (int l = 1; l <= c.bits; ++l) {
        const int cnt = c.count[l];
        for (int i = 0; i < cnt; ++i, ++idx, ++code) {
            const uint16_t e = (uint16_t)(c.perm[idx] << 4 | l);
            for (uint32_t k = infl_rev(code, l); k < (uint32_t)size; k += 1u << l) c.table[k] = e;
        }
        code <<= 1;
    }
    return 0;
}

// The symbol at the front of `buf` and the bits of its code (`used`, which may exceed what the buffer holds: the caller checks), or -1.
INFL_HD int infl_sym(const InflCode& c, uint64_t buf, int& used) {
    const uint16_t e = c.table[(uint32_t)buf & ((1u << c.bits) - 1u)];
    if (e) { used = e & 15; return e >> 4; }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; ++l) {
        code |= (int)((buf >> (l - 1)) & 1u);
        const int cnt = c.count[l];
        if (code - cnt < first) { used = l; return c.perm[index + (code - first)]; }
        index += cnt; first += cnt;
        first <<= 1; code <<= 1;
    }
    used = 1;
    return -1;
}

INFL_HD void infl_build_fixed(const InflTables& T) {
    for (int s = 0; s < 288; ++s) T.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    infl_build(T.fix_lit, T.lens, 288, false, T.offs);
    for (int s = 0; s < 32; ++s) T.lens[s] = 5;
    infl_build(T.fix_dist, T.lens, 32, false, T.offs);
}

// A dynamic block's header, behind BTYPE: 0, or INFL_EV_MORE / SHORT / INVALID.
INFL_HD int infl_dynamic_header(const InflIn& in, InflBits& b, const InflTables& T) {
    int rc = infl_need(in, b, 14); if (rc) return rc;
    const int nlen = (int)infl_take(b, 5) + 257, ndist = (int)infl_take(b, 5) + 1, ncode = (int)infl_take(b, 4) + 4;
    if (nlen > 286 || ndist > 30) return INFL_EV_INVALID;
    for (int i = 0; i < 19; ++i) T.lens[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        rc = infl_need(in, b, 3); if (rc) return rc;
        // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        const int order = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 9 - (i >> 1) : 6 + (i >> 1);
        T.lens[order] = (uint8_t)infl_take(b, 3);
    }
    if (infl_build(T.cl, T.lens, 19, false, T.offs)) return INFL_EV_INVALID;
    if (T.cl.count[0] == 19) return INFL_EV_INVALID;            // (zlib reads on and then misses the end-of-block code: rejected all the same)
    const int total = nlen + ndist;
    int have = 0;
    while (have < total) {
        rc = infl_need(in, b, 7 + 7);
        if (rc == INFL_EV_MORE) return rc;                       // (at the stream's end the bits that are there decide)
        int used;
        const int s = infl_sym(T.cl, b.buf, used);
        if (used > b.n) return INFL_EV_SHORT;
        if (s < 0) return INFL_EV_INVALID;
        const int eb = s < 16 ? 0 : s == 16 ? 2 : s == 17 ? 3 : 7;
        if (used + eb > b.n) return INFL_EV_SHORT;
        infl_take(b, used);
        if (s < 16) { T.lens[have++] = (uint8_t)s; continue; }
        int rep, val = 0;
        if (s == 16) {
            if (have == 0) return INFL_EV_INVALID;
            val = T.lens[have - 1];
            rep = 3 + (int)infl_take(b, 2);
        } else if (s == 17) rep = 3 + (int)infl_take(b, 3);
        else rep = 11 + (int)infl_take(b, 7);
        if (have + rep > total) return INFL_EV_INVALID;
        while (rep--) T.lens[have++] = (uint8_t)val;
    }
    if (T.lens[256] == 0) return INFL_EV_INVALID;               // no end-of-block code
    if (infl_build(T.dyn_lit, T.lens, nlen, true, T.offs)) return INFL_EV_INVALID;
    if (infl_build(T.dyn_dist, T.lens + nlen, ndist, true, T.offs)) return INFL_EV_INVALID;
    return 0;
}

// The next token of the stream (>= 0), or an INFL_EV_* word.  `avail`: bytes the stream has produced so far (a distance beyond them is
// invalid).  INFL_EV_MORE leaves the state as it was before the call.  Every call that returns a token or moves to another block has
// consumed at least one bit, so a caller's loop is bounded by the stream's bit count.
INFL_HD int inflate_next(const InflIn& in, InflState& st, const InflTables& T, uint32_t avail) {
    for (;;) {
        const InflBits save = st.b;
        int rc;
        if (st.mode == 2 || st.mode == 3) {
            const InflCode& lit = st.mode == 2 ? T.fix_lit : T.dyn_lit;
            const InflCode& dst = st.mode == 2 ? T.fix_dist : T.dyn_dist;
            if (st.b.n < 32) infl_refill(in, st.b);
            if (st.b.n < 20 && infl_more(in, st.b)) { infl_refill(in, st.b); if (st.b.n < 20) { st.b = save; return INFL_EV_MORE; } }
            int used;
            int s = infl_sym(lit, st.b.buf, used);
            if (used > st.b.n) return INFL_EV_SHORT;
            if (s < 0) return INFL_EV_INVALID;
            infl_take(st.b, used);
            if (s < 256) return s;
            if (s == 256) { st.mode = st.final ? 4 : 1; continue; }
            if (s > 285) return INFL_EV_INVALID;
            int len;
            if (s < 265) len = s - 254;
            else if (s == 285) len = 258;
            else {
                const int eb = (s - 261) >> 2;
                if (eb > st.b.n) return INFL_EV_SHORT;              // (20 bits were there unless the stream ends)
                len = 3 + ((4 + ((s - 261) & 3)) << eb) + (int)infl_take(st.b, eb);
            }
            if (st.b.n < 32) infl_refill(in, st.b);
            if (st.b.n < 28 && infl_more(in, st.b)) { infl_refill(in, st.b); if (st.b.n < 28) { st.b = save; return INFL_EV_MORE; } }
            s = infl_sym(dst, st.b.buf, used);
            if (used > st.b.n) return INFL_EV_SHORT;
            if (s < 0 || s > 29) return INFL_EV_INVALID;
            infl_take(st.b, used);
            uint32_t dist;
            if (s < 4) dist = (uint32_t)s + 1u;
            else {
                const int eb = (s >> 1) - 1;
                if (eb > st.b.n) return INFL_EV_SHORT;
                dist = 1u + ((2u + (uint32_t)(s & 1)) << eb) + infl_take(st.b, eb);
            }
            if (dist > avail) return INFL_EV_INVALID;
            return INFL_TOK_MATCH | len << 16 | (int)dist;
        }
        if (st.mode == 1) {
            rc = infl_need(in, st.b, 3);
            if (rc) { st.b = save; return rc; }
            st.final = (int)infl_take(st.b, 1);
            const int type = (int)infl_take(st.b, 2);
            if (type == 3) return INFL_EV_INVALID;
            if (type == 1) { st.mode = 2; continue; }
            if (type == 2) {
                rc = infl_dynamic_header(in, st.b, T);
                if (rc == INFL_EV_MORE) { st.b = save; return rc; }
                if (rc) return rc;
                st.mode = 3;
                continue;
            }
            infl_take(st.b, st.b.n & 7);                            // to the byte boundary
            rc = infl_need(in, st.b, 32);
            if (rc) { st.b = save; return rc; }
            const uint32_t v = infl_take(st.b, 32);
            if ((v & 0xffffu) != ((v >> 16) ^ 0xffffu)) return INFL_EV_INVALID;
            st.b.pos -= (uint32_t)(st.b.n >> 3);                    // whole bytes wait in the buffer: hand them back
            st.b.n = 0; st.b.buf = 0;
            st.stored_len = v & 0xffffu;
            if (st.stored_len > in.nend - st.b.pos) return INFL_EV_SHORT;
            return INFL_EV_STORED;
        }
        if (st.mode == 0) {
            rc = infl_need(in, st.b, 16);
            if (rc) { st.b = save; return rc; }
            const uint32_t cmf = infl_take(st.b, 8), flg = infl_take(st.b, 8);
            if ((cmf * 256u + flg) % 31u != 0u || (cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 0x20u)) return INFL_EV_INVALID;
            st.mode = 1;
            continue;
        }
        if (st.mode == 4) {
            InflBits b = st.b;
            infl_take(b, b.n & 7);
            rc = infl_need(in, b, 32);
            if (rc) return rc;                                      // (st.b untouched)
            const uint32_t v = infl_take(b, 32);
            st.b = b;
            st.adler = (v & 0xffu) << 24 | (v & 0xff00u) << 8 | (v >> 8 & 0xff00u) | v >> 24;
            st.mode = 5;
            return INFL_EV_DONE;
        }
        return INFL_EV_DONE;
    }
}

INFL_HD void inflate_stored_done(InflState& st) {      // the caller has copied the stored block's bytes
    st.b.pos += st.stored_len;
    st.stored_len = 0;
    st.mode = st.final ? 4 : 1;
}

INFL_HD int infl_status_of(int ev) { return ev == INFL_EV_SHORT ? INFL_SHORT : INFL_INVALID; }

// ---- one long stream on many waves (rdr_inflate_decode_split) ----------------------------------------------------------------------
// A CANDIDATE of a stream is a stream offset p, 6 <= p <= bytes - 6 (behind the zlib header and a block header, in front of the shortest
// block and the trailer), with src[p - 4 .. p) == 00 00 FF FF: the LEN / NLEN words of an empty stored block, which is what
// Z_SYNC_FLUSH, Z_FULL_FLUSH and this project's encoder leave behind - and what four bytes of
// stored data or of a Huffman code may spell by chance.  The candidate rule, deterministic: the stream is cut into windows of INFL_GAP
// bytes, window j = [j * INFL_GAP, (j + 1) * INFL_GAP), and of the candidates of one window only the FIRST and the LAST (the smallest and
// the largest p) are kept - a dependent flush point and an independent one often lie a few dozen bytes apart.  A stream of n bytes so
// has 2 (n / INFL_GAP + 1) candidate slots, and with the stream's start in front one more: slot 0 is the start, slot 1 + 2 j holds the
// first candidate p of window j, slot 2 + 2 j the complement ~p of the last one, an empty slot 0xffffffff (infl_candidate() reads them;
// the slots are in ascending order by construction).  A dropped true flush point only makes a piece longer.
//
// A PIECE starts at a slot - at the zlib header for slot 0, at a block header with an empty bit buffer for a candidate - and is
// measured without its history (infl_measure_run): it ends where a stored block ends, a block header is next and the input position is
// a later kept candidate (its successor), or at the stream's trailer, or at an error.  Only a stored block leaves the reader at a byte
// boundary with an empty bit buffer, so that is the one place where a piece that starts there reads exactly what the whole stream's
// reader reads.  A candidate the position passes without landing on it was false for this piece.  `reach` is how far the piece's
// matches look behind its own first byte: the largest dist - (bytes the piece had produced before the match), 0 if none does.
enum { INFL_GAP = 1024,
       INFL_P_NEXT = 0,           // the piece ended at its successor, the candidate at stream offset `end`
       INFL_P_FINAL = 1,          // the final block ended and the trailer was read (`adler`)
       INFL_P_BAD = 2 };          // an error, or more output than the slot takes
struct InflPiece { uint32_t start, end, produced, reach, adler; int32_t status; };      // (a slot that holds no candidate stays all ones)
// what one wave decodes: the bytes of stream `seg` from input offset `pos` (0: the zlib header comes first) up to `end` (0xffffffff: the
// trailer), into [out, out + len) of the slot.  adler: the trailer's word (the last job of a stream).
struct InflJob { int32_t seg; uint32_t pos, end, out, len, last, adler; };
struct InflJobOut { uint32_t A, B, len; int32_t status; };           // the piece's own Adler-32 sums (from A = 1, B = 0), bytes written

// A stream's length and a slot's size as the kernels take them (infl_segment clips to the same bound): the host's plan and the
// device's passes agree on both by construction.
enum : int64_t { INFL_MAX_BYTES = 0x7fffff00LL };
INFL_HD uint32_t infl_clip32(int64_t v) { return (uint32_t)(v < 0 ? 0 : v > INFL_MAX_BYTES ? INFL_MAX_BYTES : v); }
INFL_HD uint32_t infl_slots(uint32_t nbytes) { return 1u + 2u * (nbytes / (uint32_t)INFL_GAP + 1u); }
// the candidate of slot k of cand (the stream's candidate slots, infl_slots() - 1 of them), or 0xffffffff: none (a last that is the first too)
INFL_HD uint32_t infl_candidate(const uint32_t* cand, uint32_t k) {
    const uint32_t v = cand[k];
    if (!(k & 1u) || v == 0xffffffffu) return v;
    return ~v == cand[k - 1u] ? 0xffffffffu : ~v;
}
// the slot of cand that holds stream offset p, or 0xffffffff: p is no kept candidate
INFL_HD uint32_t infl_candidate_slot(const uint32_t* cand, uint32_t ncand, uint32_t p) {
    const uint32_t k = 2u * (p / (uint32_t)INFL_GAP);
    if (k + 1u >= ncand || p == 0xffffffffu) return 0xffffffffu;
    return cand[k] == p ? k : cand[k + 1u] == ~p ? k + 1u : 0xffffffffu;
}

// Lane 0's part of the measure pass, and the host probe's: tokens are decoded and counted, nothing is written.  m: the stream's global
// address mod 4, cap: the slot's size.  Returns 0 when the piece has ended (P.status is set), 1 when the window has to be staged again at
// st.b.pos first.  The caller bounds the number of calls (every call that returns 1 has consumed a bit or is followed by one that does).
INFL_HD int infl_measure_run(const InflIn& in, InflState& st, const InflTables& T, uint32_t m, uint32_t cap, const uint32_t* cand, uint32_t ncand, InflPiece& P) {
    for (;;) {
        if (infl_restage(in, st.b.pos, false, false)) return 1;
        const int t = inflate_next(in, st, T, 0xffffffffu);         // (no distance is too far here: `reach` records it, the plan decides)
        if (t >= 0) {
            const uint32_t len = (uint32_t)infl_tok_len(t);
            if (len > cap - P.produced) { P.status = INFL_P_BAD; return 0; }
            if (t & INFL_TOK_MATCH) {
                const uint32_t dist = (uint32_t)infl_tok_dist(t);
                if (dist > P.produced && dist - P.produced > P.reach) P.reach = dist - P.produced;
            }
            P.produced += len;
            continue;
        }
        if (t == INFL_EV_MORE) return 1;
        if (t == INFL_EV_STORED) {
            if (st.stored_len > cap - P.produced) { P.status = INFL_P_BAD; return 0; }
            P.produced += st.stored_len;
            inflate_stored_done(st);
            const uint32_t p = st.b.pos - m;
            if (st.mode == 1 && p > P.start && infl_candidate_slot(cand, ncand, p) != 0xffffffffu) { P.end = p; P.status = INFL_P_NEXT; return 0; }
            continue;
        }
        if (t == INFL_EV_DONE) { P.adler = st.adler; P.end = 0xffffffffu; P.status = INFL_P_FINAL; return 0; }
        P.status = INFL_P_BAD;
        return 0;
    }
}

// The plan of one stream, from the records of its slots (rec[0]: the start).  Follows the chain of successors from the start and writes
// the jobs of the stream's final pieces to jobs[0 .. return value), which needs room for `nslots`; 0: the stream is not provably clean
// and goes to inflate_kernel.  Piece k opens a job of its own when its reach is 0 and it has output (the empty final block behind a
// last flush point is no work for a wave); otherwise it joins the job before it, and that job
// is joined with the one before it for as long as the output since the job's start is below reach_k - so every member of a job finds
// its whole reach inside the job (members that joined earlier keep theirs: a job's start only moves back).  Clean: the chain ends at
// the trailer, no piece of it is bad, the total fits the slot, and no reach exceeds the output before the piece (zlib's "distance too
// far back").
INFL_HD uint32_t infl_plan(const InflPiece* rec, uint32_t nslots, uint32_t cap, int32_t seg, InflJob* jobs) {
    uint32_t k = 0, n = 0;
    uint64_t total = 0;
    for (;;) {
        const InflPiece& r = rec[k];
        if (r.status != INFL_P_NEXT && r.status != INFL_P_FINAL) return 0;
        if (r.reach > total) return 0;
        if (k == 0 || (r.reach == 0 && r.produced != 0)) {
            jobs[n++] = InflJob{seg, r.start, 0xffffffffu, (uint32_t)total, 0u, 0u, 0u};
        } else
            while (n > 1 && r.reach > total - jobs[n - 1].out) --n;     // (jobs[0].out == 0 and reach <= total)
        total += r.produced;
        if (total > cap) return 0;
        if (r.status == INFL_P_FINAL) { jobs[n - 1].adler = r.adler; break; }
        uint32_t j = 1u + 2u * (r.end / (uint32_t)INFL_GAP);                 // the window's first candidate, or its last
        if (j + 1u >= nslots) return 0;
        if (rec[j].start != r.end) ++j;
        if (j <= k || rec[j].start != r.end) return 0;
        k = j;
    }
    for (uint32_t i = 0; i + 1 < n; ++i) { jobs[i].end = jobs[i + 1].pos; jobs[i].len = jobs[i + 1].out - jobs[i].out; }
    jobs[n - 1].len = (uint32_t)total - jobs[n - 1].out;
    jobs[n - 1].last = 1u;
    return n;
}

// Adler-32 of a concatenation: (A, B) of the bytes so far, then a piece of len2 bytes with its own sums (A2, B2).
INFL_HD void infl_adler_fold(uint32_t& A, uint32_t& B, uint32_t A2, uint32_t B2, uint32_t len2) {
    const uint32_t a1 = (A + 65520u) % 65521u;                           // A - 1
    B = (uint32_t)((B + B2 + (uint64_t)(len2 % 65521u) * a1) % 65521u);
    A = (A + A2 + 65520u) % 65521u;
}

#ifdef __HIPCC__

// The output offset up to which whole words of the global address can be flushed, or `flushed` when no word boundary lies behind it
// (with align + produced < 4 the difference below would wrap).
__device__ __forceinline__ uint32_t infl_words_upto(uint32_t align, uint32_t produced, uint32_t flushed) {
    const uint32_t q = (align + produced) & ~3u;
    return q > align + flushed ? q - align : flushed;
}

// Output positions [lo, hi) of the ring -> dst, and their Adler-32 sums folded into (A, B).  q = align + position is congruent to the
// global address mod 4.  Lane l sums the bytes it stores; the wave sums are those of deflate_kernels.h (s1 = sum b, s2 = sum (n - i) b).
__device__ __forceinline__ void infl_flush(const uint8_t* ring, uint8_t* dst, uint32_t align, uint32_t lo, uint32_t hi, int lane, uint32_t& A, uint32_t& B) {
    if (lo >= hi) return;
    const uint32_t qlo = align + lo, qhi = align + hi, n = hi - lo;
    const uint32_t wlo = (qlo + 3u) & ~3u, whi = qhi & ~3u;
    uint64_t s1 = 0, s2 = 0;
    if (wlo >= whi) {
        for (uint32_t q = qlo + lane; q < qhi; q += 64) {
            const uint32_t b = ring[q & INFL_RING_MASK];
            dst[q - align] = (uint8_t)b;
            s1 += b; s2 += (uint64_t)(qhi - q) * b;
        }
    } else {
        if (qlo + lane < wlo) {
            const uint32_t q = qlo + lane, b = ring[q & INFL_RING_MASK];
            dst[q - align] = (uint8_t)b;
            s1 += b; s2 += (uint64_t)(qhi - q) * b;
        }
        for (uint32_t q = wlo + 4u * lane; q < whi; q += 256) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(ring + (q & INFL_RING_MASK));
            *reinterpret_cast<uint32_t*>(dst + (q - align)) = w;
            const uint32_t b0 = w & 255u, b1 = (w >> 8) & 255u, b2 = (w >> 16) & 255u, b3 = w >> 24, r = qhi - q;
            s1 += b0 + b1 + b2 + b3;
            s2 += (uint64_t)r * b0 + (uint64_t)(r - 1u) * b1 + (uint64_t)(r - 2u) * b2 + (uint64_t)(r - 3u) * b3;
        }
        if (whi + lane < qhi) {
            const uint32_t q = whi + lane, b = ring[q & INFL_RING_MASK];
            dst[q - align] = (uint8_t)b;
            s1 += b; s2 += (uint64_t)(qhi - q) * b;
        }
    }
    uint32_t t1 = (uint32_t)(s1 % 65521u), t2 = (uint32_t)(s2 % 65521u);
    for (int d = 1; d < 64; d <<= 1) {                                          // every lane ends with the wave's sums
        t1 += (uint32_t)__shfl_xor((int)t1, d, 64);
        t2 += (uint32_t)__shfl_xor((int)t2, d, 64);
    }
    t1 %= 65521u; t2 %= 65521u;
    B = (uint32_t)((B + (uint64_t)(n % 65521u) * A + t2) % 65521u);
    A = (A + t1) % 65521u;
}

// One stream, or one piece of one (PIECE), by the calling wave: `in` / `nbytes` the stream, dst its slot, cap the bytes of the slot that
// may be written.  PIECE: decoding starts at input offset pos0 (0: at the zlib header) and output offset out0 with an empty history and
// ends where a stored block ends at input offset `end`, or at the trailer; the Adler-32 is then the piece's own and is not compared.
// Returns the status; flushed: the output offset reached (every byte below it is stored), (A, B): the sums, adler: the trailer's word.
template <bool PIECE>
__device__ __forceinline__ int infl_decode_range(InflShared& S, const InflTables& T, int lane, const uint8_t* in, uint32_t nbytes, uint8_t* dst, uint32_t cap,
                                                 uint32_t pos0, uint32_t out0, uint32_t end, uint32_t& flushed_out, uint32_t& A_out, uint32_t& B_out, uint32_t& adler_out) {
    const uint32_t m = (uint32_t)(reinterpret_cast<uintptr_t>(in) & 3u);         // virtual input position = m + byte
    const uint32_t align = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);    // ring index == global address (mod 4)
    uint32_t adler = 0u;
    InflIn win{reinterpret_cast<const uint8_t*>(S.in), 0u, 0u, m + nbytes};
    InflState st;                                    // (lane 0's copy is the one that counts)
    inflate_init(st, m);
    if (PIECE && pos0) { st.b.pos = m + pos0; st.mode = 1; }               // a block header is next, the bit buffer is empty
    uint32_t produced = PIECE ? out0 : 0u, flushed = produced, A = 1u, B = 0u;
    uint64_t guard = 16ull * nbytes + 64ull;         // a batch consumes a bit, or restages and the next one does: a damaged stream cannot spin
    int result = -1;
    bool first = true, more = false;
    while (result < 0) {
        if (guard-- == 0) { result = INFL_INVALID; break; }
        // ---- stage the input window when little of it is left
        const uint32_t vpos = (uint32_t)__shfl((int)st.b.pos, 0, 64);
        if (infl_restage(win, vpos, first, more)) {
            infl_window(win, vpos);
            for (int k = lane; k < INFL_WIN / 4; k += 64) {
                const int64_t p0 = (int64_t)win.base + 4 * k - (int64_t)m;           // the word's first byte in the stream
                uint32_t w = 0u;
                if (p0 >= 0 && p0 + 4 <= (int64_t)nbytes) w = *reinterpret_cast<const uint32_t*>(in + p0);
                else
                    for (int j = 0; j < 4; ++j)
                        if (p0 + j >= 0 && p0 + j < (int64_t)nbytes) w |= (uint32_t)in[p0 + j] << (8 * j);
                S.in[k] = w;
            }
            first = false;
            __syncthreads();
        }
        // ---- lane 0: a batch of tokens
        if (lane == 0) {
            int n = 0, ev = 0;
            uint32_t o = produced;
            while (n < 64) {
                const int t = inflate_next(win, st, T, o);
                if (t < 0) { ev = t; break; }
                const uint32_t len = (uint32_t)infl_tok_len(t);
                if (len > cap - o) { ev = 1; break; }                                // the stream holds more than the slot
                S.tok[n] = t;
                S.off[n] = o;
                o += len;
                ++n;
            }
            if (ev == INFL_EV_STORED && st.stored_len > cap - o) ev = 1;
            S.off[n] = o;
            S.ctl[0] = (uint32_t)n; S.ctl[1] = (uint32_t)ev; S.ctl[2] = st.stored_len; S.ctl[3] = st.b.pos; S.ctl[4] = st.adler;
        }
        __syncthreads();
        const int ntok = (int)S.ctl[0] <= 64 ? (int)S.ctl[0] : 64, ev = (int)S.ctl[1];
        // ---- the wave: the batch into the ring, in token order
        {
            const int my = lane < ntok ? S.tok[lane] : 0;
            const uint32_t myq = align + (lane < ntok ? S.off[lane] : 0u);
            const uint64_t matches = __ballot(lane < ntok && (my & INFL_TOK_MATCH));
            int i = 0;
            while (i < ntok) {
                const uint64_t rem = matches >> i;
                if (rem & 1ull) {
                    const int t = S.tok[i];
                    const uint32_t q = align + S.off[i], len = (uint32_t)infl_tok_len(t), dist = (uint32_t)infl_tok_dist(t);
                    const bool self = dist < len;
                    const uint32_t dd = dist ? dist : 1u;
                    for (uint32_t k0 = 0; k0 < len; k0 += 64) {                      // (len <= 258: at most five steps)
                        const uint32_t k = k0 + lane;
                        uint8_t v = 0;
                        if (k < len) v = S.ring[(q - dist + (self ? k % dd : k)) & INFL_RING_MASK];
                        __syncthreads();                                             // every byte of the step is read before one is written
                        if (k < len) S.ring[(q + k) & INFL_RING_MASK] = v;
                        __syncthreads();
                    }
                    ++i;
                } else {
                    const int j = rem ? i + (int)__builtin_ctzll(rem) : ntok;        // the literals [i, j)
                    if (lane >= i && lane < j) S.ring[myq & INFL_RING_MASK] = (uint8_t)my;
                    __syncthreads();
                    i = j;
                }
            }
        }
        produced = S.off[ntok] <= cap ? S.off[ntok] : cap;
        more = ev == INFL_EV_MORE;
        bool piece_end = false;                                                      // (PIECE) the stored block ends where the piece does
        if (ev == INFL_EV_STORED) {
            if (PIECE) piece_end = S.ctl[3] - m + S.ctl[2] == end;
            // ---- a stored block: a cooperative copy from the input, flushed as it goes
            uint32_t left = S.ctl[2];
            uint32_t p = S.ctl[3] - m;                                               // its first byte in the stream
            if (p > nbytes || left > nbytes - p || left > cap - produced) left = 0;  // (lane 0 has checked both)
            if (left && produced > flushed) {                                        // room for the copy: at most 3 bytes wait behind this
                const uint32_t upto = infl_words_upto(align, produced, flushed);
                if (upto > flushed) { infl_flush(S.ring, dst, align, flushed, upto, lane, A, B); flushed = upto; }
                __syncthreads();
            }
            while (left) {
                const uint32_t c = left < (uint32_t)INFL_FLUSH ? left : (uint32_t)INFL_FLUSH;
                for (uint32_t k = lane; k < c; k += 64) S.ring[(align + produced + k) & INFL_RING_MASK] = in[p + k];
                __syncthreads();
                produced += c; p += c; left -= c;
                if (produced - flushed >= (uint32_t)INFL_FLUSH) {
                    const uint32_t upto = infl_words_upto(align, produced, flushed);        // whole words; the rest waits
                    if (upto > flushed) { infl_flush(S.ring, dst, align, flushed, upto, lane, A, B); flushed = upto; }
                    __syncthreads();
                }
            }
            if (lane == 0) inflate_stored_done(st);
        }
        // ---- flush: whole words while the stream goes on, everything at its end
        const bool ended = (ev != 0 && ev != INFL_EV_MORE && ev != INFL_EV_STORED) || piece_end;
        if (ended) {
            infl_flush(S.ring, dst, align, flushed, produced, lane, A, B);
            flushed = produced;
        } else if (produced - flushed >= (uint32_t)INFL_FLUSH) {
            const uint32_t upto = infl_words_upto(align, produced, flushed);
            if (upto > flushed) { infl_flush(S.ring, dst, align, flushed, upto, lane, A, B); flushed = upto; }
        }
        if (ev == INFL_EV_DONE) { adler = S.ctl[4]; result = PIECE || ((B << 16) | A) == adler ? INFL_OK : INFL_CHECKSUM; }
        else if (piece_end) result = INFL_OK;
        else if (ev == 1) result = INFL_OVERFLOW;
        else if (ended) result = infl_status_of(ev);
        __syncthreads();                                                            // (S.ctl / S.off are rewritten by the next batch)
    }
    flushed_out = flushed; A_out = A; B_out = B; adler_out = adler;
    return result;
}

// The input range of stream `seg`, clipped to the buffer, and its output slot, clipped to the stride.
struct InflSeg { const uint8_t* in; uint8_t* dst; uint32_t nbytes, cap; };
__device__ __forceinline__ InflSeg infl_segment(const uint8_t* src, int64_t src_bytes, const int64_t* seg_offset, const int64_t* seg_bytes, const int64_t* seg_out_bytes,
                                                int64_t seg, uint8_t* out, int64_t out_stride) {
    int64_t so = seg_offset[seg], sb = seg_bytes[seg], cap64 = seg_out_bytes ? seg_out_bytes[seg] : 0;
    if (so < 0 || so > src_bytes) { so = 0; sb = 0; }
    if (sb < 0) sb = 0;
    if (sb > src_bytes - so) sb = src_bytes - so;
    if (sb > INFL_MAX_BYTES) sb = INFL_MAX_BYTES;
    if (cap64 < 0) cap64 = 0;
    if (cap64 > out_stride) cap64 = out_stride;
    if (cap64 > INFL_MAX_BYTES) cap64 = INFL_MAX_BYTES;
    return InflSeg{src + so, out + seg * out_stride, (uint32_t)sb, (uint32_t)cap64};
}

// out slots are at out + i * out_stride; status[i] as INFL_*; produced[i] (may be NULL): bytes written to the slot.  list (may be NULL):
// the streams to decode, nseg of them, instead of 0 .. nseg - 1 (rdr_inflate_decode_split's streams that stay whole).
__global__ __launch_bounds__(64) void inflate_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ seg_offset,
                                                    const int64_t* __restrict__ seg_bytes, const int64_t* __restrict__ seg_out_bytes, int nseg,
                                                    uint8_t* __restrict__ out, int64_t out_stride, int32_t* __restrict__ status, int64_t* __restrict__ produced_out,
                                                    const int32_t* __restrict__ list) {
    __shared__ __attribute__((aligned(16))) InflShared S;
    const InflTables T = infl_tables(S);
    const int lane = threadIdx.x;
    if (lane == 0) infl_build_fixed(T);
    __syncthreads();
    for (int k = blockIdx.x; k < nseg; k += gridDim.x) {
        const int seg = list ? list[k] : k;
        const InflSeg G = infl_segment(src, src_bytes, seg_offset, seg_bytes, seg_out_bytes, seg, out, out_stride);
        uint32_t flushed, A, B, adler;
        const int result = infl_decode_range<false>(S, T, lane, G.in, G.nbytes, G.dst, G.cap, 0u, 0u, 0u, flushed, A, B, adler);
        if (lane == 0) {
            status[seg] = result;
            if (produced_out) produced_out[seg] = (int64_t)flushed;
        }
        __syncthreads();
    }
}

// ---- rdr_inflate_decode_split: scan, measure, (plan on the host), pieces, fold ------------------------------------------------------
// Every candidate of every stream: of window j = p / INFL_GAP, cand[base[seg] + 1 + 2 j] = the smallest p and cand[base[seg] + 2 + 2 j] = the
// complement of the largest (cand is all ones before), and count[seg] = the windows of the stream that hold one.  Integer vector atomics only; the slots are in ascending order by construction.
__global__ __launch_bounds__(256) void infl_scan_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ seg_offset,
                                                        const int64_t* __restrict__ seg_bytes, int nseg, const int64_t* __restrict__ base, int64_t total_slots,
                                                        uint32_t* __restrict__ cand, uint32_t* __restrict__ count) {
    for (int seg = blockIdx.y; seg < nseg; seg += gridDim.y) {
        const InflSeg G = infl_segment(src, src_bytes, seg_offset, seg_bytes, nullptr, seg, nullptr, 0);
        const int64_t n = G.nbytes, b0 = base[seg] + 1;
        for (int64_t p = 6 + (int64_t)blockIdx.x * 256 + threadIdx.x; p <= n - 6; p += (int64_t)gridDim.x * 256) {
            if (G.in[p - 4] != 0u || G.in[p - 3] != 0u || G.in[p - 2] != 0xffu || G.in[p - 1] != 0xffu) continue;
            const int64_t slot = b0 + 2 * (p / INFL_GAP);
            if (slot + 1 >= base[seg + 1] || slot + 1 >= total_slots) continue;         // (cannot happen: base is built from the same sizes)
            if (atomicMin(&cand[slot], (uint32_t)p) == 0xffffffffu) atomicAdd(&count[seg], 1u);
            atomicMin(&cand[slot + 1], ~(uint32_t)p);
        }
    }
}

struct InflMeasureShared {        // InflShared without the ring and the token batch: 10.3 KiB, so the measure pass runs 15 workgroups per compute unit
    uint32_t in[INFL_WIN / 4];
    uint16_t fix_lit[1 << INFL_LBITS], fix_dist[1 << INFL_DBITS], dyn_lit[1 << INFL_LBITS], dyn_dist[1 << INFL_DBITS];
    uint16_t fix_lit_perm[288], fix_dist_perm[32], dyn_lit_perm[288], dyn_dist_perm[32];
    uint16_t cl_table[1 << INFL_CBITS], cl_perm[20];
    uint16_t counts[5][16];
    uint16_t offs[16];
    uint8_t lens[320];
    uint32_t ctl[2];
};

// One wave per slot of the streams that hold a candidate: rec[slot] = the piece that starts there (a slot without a candidate keeps its
// all-ones record).  Lane 0 decodes, the wave stages the input window.
__global__ __launch_bounds__(64) void infl_measure_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ seg_offset,
                                                         const int64_t* __restrict__ seg_bytes, const int64_t* __restrict__ seg_out_bytes, int nseg, int64_t out_stride,
                                                         const int64_t* __restrict__ base, int64_t total_slots, const uint32_t* __restrict__ cand,
                                                         const uint32_t* __restrict__ count, InflPiece* __restrict__ rec) {
    __shared__ __attribute__((aligned(16))) InflMeasureShared S;
    const InflTables T = infl_tables(S);
    const int lane = threadIdx.x;
    if (lane == 0) infl_build_fixed(T);
    __syncthreads();
    for (int64_t slot = blockIdx.x; slot < total_slots; slot += gridDim.x) {
        int lo = 0, hi = nseg - 1;                                                      // the stream of the slot: the last one with base <= slot
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (base[mid] <= slot) lo = mid; else hi = mid - 1;
        }
        const int seg = lo;
        if (count[seg] == 0u) continue;                                                 // (uniform over the wave, as everything up to the loop is)
        const int64_t j = slot - base[seg];
        const uint32_t start = j == 0 ? 0u : infl_candidate(cand + base[seg] + 1, (uint32_t)(j - 1));
        if (start == 0xffffffffu) continue;
        const InflSeg G = infl_segment(src, src_bytes, seg_offset, seg_bytes, seg_out_bytes, seg, nullptr, out_stride);
        if (start > G.nbytes) continue;
        const uint32_t ncand = (uint32_t)(base[seg + 1] - base[seg] - 1);
        const uint32_t m = (uint32_t)(reinterpret_cast<uintptr_t>(G.in) & 3u);
        InflIn win{reinterpret_cast<const uint8_t*>(S.in), 0u, 0u, m + G.nbytes};
        InflState st;
        inflate_init(st, m);
        if (j) { st.b.pos = m + start; st.mode = 1; }
        InflPiece P{start, 0u, 0u, 0u, 0u, INFL_P_BAD};
        uint64_t guard = 16ull * G.nbytes + 64ull;
        for (;;) {
            const uint32_t vpos = (uint32_t)__shfl((int)st.b.pos, 0, 64);
            infl_window(win, vpos);
            for (int k = lane; k < INFL_WIN / 4; k += 64) {
                const int64_t p0 = (int64_t)win.base + 4 * k - (int64_t)m;
                uint32_t w = 0u;
                if (p0 >= 0 && p0 + 4 <= (int64_t)G.nbytes) w = *reinterpret_cast<const uint32_t*>(G.in + p0);
                else
                    for (int b = 0; b < 4; ++b)
                        if (p0 + b >= 0 && p0 + b < (int64_t)G.nbytes) w |= (uint32_t)G.in[p0 + b] << (8 * b);
                S.in[k] = w;
            }
            __syncthreads();
            if (lane == 0) {
                int again = 0;
                if (guard-- == 0) P.status = INFL_P_BAD;
                else again = infl_measure_run(win, st, T, m, G.cap, cand + base[seg] + 1, ncand, P);
                S.ctl[0] = (uint32_t)again;
            }
            __syncthreads();
            const uint32_t again = S.ctl[0];
            __syncthreads();                                                            // (S.in and S.ctl are rewritten by the next round)
            if (!again) break;
        }
        if (lane == 0) rec[slot] = P;
    }
}

// One wave per job.  res[j]: the piece's own Adler-32 sums and the bytes it wrote; a job that does not fit its stream is refused.
// A piece that does not end where and as the measure pass recorded it gets INFL_INVALID, which the fold hands on: an INTERNAL-CONSISTENCY
// status, not a verdict on the stream - both passes run inflate_next() over the same bytes from the same state, so it cannot arise from
// any input, and it is not one of the outcomes the serial call's contract covers.
__global__ __launch_bounds__(64) void inflate_piece_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int64_t* __restrict__ seg_offset,
                                                          const int64_t* __restrict__ seg_bytes, const int64_t* __restrict__ seg_out_bytes, int nseg,
                                                          uint8_t* __restrict__ out, int64_t out_stride, const InflJob* __restrict__ jobs, int64_t njobs,
                                                          InflJobOut* __restrict__ res) {
    __shared__ __attribute__((aligned(16))) InflShared S;
    const InflTables T = infl_tables(S);
    const int lane = threadIdx.x;
    if (lane == 0) infl_build_fixed(T);
    __syncthreads();
    for (int64_t k = blockIdx.x; k < njobs; k += gridDim.x) {
        const InflJob J = jobs[k];
        InflJobOut R{1u, 0u, 0u, INFL_INVALID};
        if (J.seg >= 0 && J.seg < nseg) {
            const InflSeg G = infl_segment(src, src_bytes, seg_offset, seg_bytes, seg_out_bytes, J.seg, out, out_stride);
            if (J.pos <= G.nbytes && J.out <= G.cap && J.len <= G.cap - J.out) {
                uint32_t flushed, adler;
                R.status = infl_decode_range<true>(S, T, lane, G.in, G.nbytes, G.dst, J.out + J.len, J.pos, J.out, J.end, flushed, R.A, R.B, adler);
                R.len = flushed - J.out;
                if (R.len != J.len || (J.last && adler != J.adler)) R.status = INFL_INVALID;        // (the measure pass saw the same bytes)
            }
        }
        if (lane == 0) res[k] = R;
        __syncthreads();
    }
}

// One thread per job; the one that holds a stream's last job folds the stream's pieces in order and writes its status.
__global__ __launch_bounds__(256) void infl_fold_kernel(const InflJob* __restrict__ jobs, const InflJobOut* __restrict__ res, int64_t njobs, int nseg,
                                                        int32_t* __restrict__ status, int64_t* __restrict__ produced_out) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < njobs; k += (int64_t)gridDim.x * 256) {
        if (!jobs[k].last) continue;
        const int32_t seg = jobs[k].seg;
        if (seg < 0 || seg >= nseg) continue;
        int64_t k0 = k;
        while (k0 > 0 && jobs[k0 - 1].seg == seg) --k0;
        uint32_t A = 1u, B = 0u;
        int64_t total = 0;
        bool ok = true;
        for (int64_t i = k0; i <= k; ++i) {
            ok = ok && res[i].status == INFL_OK;
            infl_adler_fold(A, B, res[i].A, res[i].B, res[i].len);
            total += res[i].len;
        }
        status[seg] = !ok ? INFL_INVALID : ((B << 16) | A) == jobs[k].adler ? INFL_OK : INFL_CHECKSUM;
        if (produced_out) produced_out[seg] = total;
    }
}

// ---- the inverse of h5_chunks_kernel ---------------------------------------------------------------------------------------------
struct H5UnchunkLayout : H5ChunkGrid {             // (deflate_kernels.h; total_elems counts the PRESENT chunks)
    int64_t chunk_stride;                          // bytes between decoded chunks
    int es, shuffle, swap;
};

__global__ __launch_bounds__(256) void h5_unchunk_kernel(const uint8_t* __restrict__ chunks, const int64_t* __restrict__ index, H5UnchunkLayout L,
                                                         uint8_t* __restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < L.total_elems; e += (int64_t)gridDim.x * 256) {
        const int64_t k = e / L.chunk_elems, i = e % L.chunk_elems;
        int64_t ci = index[k], ii = i;
        bool inside = true;
        int64_t idx[4];
        for (int d = 3; d >= 0; --d) {
            const int64_t x = (ci % L.nchunk[d]) * L.chunk[d] + ii % L.chunk[d];
            ci /= L.nchunk[d]; ii /= L.chunk[d];
            idx[d] = x;
            inside = inside && x < L.shape[d];
        }
        if (!inside || ci != 0) continue;                                               // edge padding; (an index beyond the grid: checked on the host)
        const int64_t dst = ((idx[0] * L.shape[1] + idx[1]) * L.shape[2] + idx[2]) * L.shape[3] + idx[3];
        const uint8_t* c = chunks + k * L.chunk_stride;
        for (int j = 0; j < L.es; ++j) {
            const uint8_t b = L.shuffle ? c[(int64_t)j * L.chunk_elems + i] : c[i * L.es + j];
            out[dst * L.es + (L.swap ? L.es - 1 - j : j)] = b;
        }
    }
}

#endif  // __HIPCC__

}  // namespace rdr
