// inflate_host_check - the bit reader, the table builder and the token decoder of raider_amd/csrc/inflate_kernels.h (the __host__
// __device__ functions lane 0 of the device kernel runs) on the CPU, over zlib streams read from a file, for a build with
// -fsanitize=address,undefined:
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/probes/inflate_host_check.cpp -o inflate_host_check
//   ./inflate_host_check streams.bin
//
// streams.bin: u32 count, then per stream u32 input bytes, u32 output capacity, the input bytes (little-endian).  Input and output live
// in heap blocks of exactly those sizes, so any access outside a stream's own bytes is a sanitizer report.  Prints one line per
// stream: status (RDR_INFL_*), bytes produced, CRC-32 of the output, tokens decoded.  No GPU call is made.
//
// Every stream is decoded five times: once with the whole stream as the window, and once at each of the four source alignments the way
// the kernel reads it - a staged window of INFL_WIN bytes (a heap block of exactly that size), batches of at most 64 tokens, the
// kernel's own restage rule (infl_restage / infl_window) before every batch - so that INFL_EV_MORE, the state restore and the restage
// run under the sanitizers too.  The five results must agree; a difference is reported on stderr and the exit status is 3.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../raider_amd/csrc/inflate_kernels.h"

using namespace rdr;

static int decode(InflShared& S, const uint8_t* in, uint32_t nbytes, uint8_t* out, uint32_t cap, uint32_t* produced_out, uint64_t* tokens_out) {
    const InflTables T = infl_tables(S);
    const InflIn win{in, 0u, nbytes, nbytes};              // the window is the stream: INFL_EV_MORE cannot happen
    InflState st;
    inflate_init(st, 0u);
    uint32_t o = 0, A = 1u, B = 0u;
    uint64_t tokens = 0;
    int result = -1;
    while (result < 0) {
        const int t = inflate_next(win, st, T, o);
        if (t >= 0) {
            const uint32_t len = (uint32_t)infl_tok_len(t);
            if (len > cap - o) { result = INFL_OVERFLOW; break; }
            ++tokens;
            if (t & INFL_TOK_MATCH) {
                const uint32_t dist = (uint32_t)infl_tok_dist(t);
                for (uint32_t k = 0; k < len; ++k) out[o + k] = out[o + k - dist];
            } else
                out[o] = (uint8_t)t;
            o += len;
        } else if (t == INFL_EV_STORED) {
            if (st.stored_len > cap - o) { result = INFL_OVERFLOW; break; }
            if (st.stored_len) std::memcpy(out + o, in + st.b.pos, st.stored_len);
            o += st.stored_len;
            inflate_stored_done(st);
        } else if (t == INFL_EV_DONE) {
            for (uint32_t k = 0; k < o; ++k) { A = (A + out[k]) % 65521u; B = (B + A) % 65521u; }
            result = ((B << 16) | A) == st.adler ? INFL_OK : INFL_CHECKSUM;
        } else if (t == INFL_EV_MORE)
            result = INFL_INVALID;                         // (cannot happen)
        else
            result = infl_status_of(t);
    }
    *produced_out = o;
    *tokens_out = tokens;
    return result;
}

// The kernel's staging and batch loop around the same functions; m: the stream's global address mod 4.
static int decode_windowed(InflShared& S, const uint8_t* in, uint32_t nbytes, uint8_t* out, uint32_t cap, uint32_t m, uint32_t* produced_out, uint64_t* tokens_out) {
    const InflTables T = infl_tables(S);
    uint8_t* stage = (uint8_t*)std::malloc(INFL_WIN);
    InflIn win{stage, 0u, 0u, m + nbytes};
    InflState st;
    inflate_init(st, m);
    uint32_t o = 0, A = 1u, B = 0u;
    uint64_t tokens = 0, guard = 16ull * nbytes + 64ull;
    int result = -1;
    bool first = true, more = false;
    while (result < 0) {
        if (guard-- == 0) { result = INFL_INVALID; break; }
        if (infl_restage(win, st.b.pos, first, more)) {
            infl_window(win, st.b.pos);
            for (uint32_t i = 0; i < (uint32_t)INFL_WIN; ++i) {
                const int64_t p = (int64_t)win.base + i - (int64_t)m;
                stage[i] = (p >= 0 && p < (int64_t)nbytes) ? in[p] : (uint8_t)0;
            }
            first = false;
        }
        int n = 0, ev = 0;
        while (n < 64) {
            const int t = inflate_next(win, st, T, o);
            if (t < 0) { ev = t; break; }
            const uint32_t len = (uint32_t)infl_tok_len(t);
            if (len > cap - o) { ev = 1; break; }
            if (t & INFL_TOK_MATCH) {
                const uint32_t dist = (uint32_t)infl_tok_dist(t);
                for (uint32_t k = 0; k < len; ++k) out[o + k] = out[o + k - dist];
            } else
                out[o] = (uint8_t)t;
            o += len;
            ++n; ++tokens;
        }
        more = ev == INFL_EV_MORE;
        if (ev == INFL_EV_STORED) {
            if (st.stored_len > cap - o) ev = 1;
            else {
                if (st.stored_len) std::memcpy(out + o, in + (st.b.pos - m), st.stored_len);
                o += st.stored_len;
                inflate_stored_done(st);
            }
        }
        if (ev == INFL_EV_DONE) {
            for (uint32_t k = 0; k < o; ++k) { A = (A + out[k]) % 65521u; B = (B + A) % 65521u; }
            result = ((B << 16) | A) == st.adler ? INFL_OK : INFL_CHECKSUM;
        } else if (ev == 1) result = INFL_OVERFLOW;
        else if (ev != 0 && ev != INFL_EV_MORE && ev != INFL_EV_STORED) result = infl_status_of(ev);
    }
    std::free(stage);
    *produced_out = o;
    *tokens_out = tokens;
    return result;
}

static uint32_t crc32_of(const uint8_t* p, uint32_t n) {           // CRC-32 as zlib.crc32 has it
    uint32_t h = 0xffffffffu;
    for (uint32_t k = 0; k < n; ++k) {
        h ^= p[k];
        for (int j = 0; j < 8; ++j) h = (h >> 1) ^ (0xedb88320u & (0u - (h & 1u)));
    }
    return h ^ 0xffffffffu;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s streams.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    InflShared* S = (InflShared*)std::malloc(sizeof(InflShared));
    std::memset(S, 0, sizeof(InflShared));
    infl_build_fixed(infl_tables(*S));
    uint32_t n = 0;
    int differ = 0;
    if (std::fread(&n, 4, 1, f) != 1) return 2;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t hdr[2];
        if (std::fread(hdr, 4, 2, f) != 2) return 2;
        uint8_t* in = (uint8_t*)std::malloc(hdr[0] ? hdr[0] : 1);
        uint8_t* out = (uint8_t*)std::malloc(hdr[1] ? hdr[1] : 1);
        if (hdr[0] && std::fread(in, 1, hdr[0], f) != hdr[0]) return 2;
        std::memset(out, 0, hdr[1] ? hdr[1] : 1);
        uint32_t produced = 0;
        uint64_t tokens = 0;
        const int status = decode(*S, in, hdr[0], out, hdr[1], &produced, &tokens);
        const uint32_t h = crc32_of(out, produced);
        std::printf("%d %u %08x %llu\n", status, produced, h, (unsigned long long)tokens);
        for (uint32_t m = 0; m < 4; ++m) {
            uint8_t* out2 = (uint8_t*)std::malloc(hdr[1] ? hdr[1] : 1);
            std::memset(out2, 0, hdr[1] ? hdr[1] : 1);
            uint32_t produced2 = 0;
            uint64_t tokens2 = 0;
            const int status2 = decode_windowed(*S, in, hdr[0], out2, hdr[1], m, &produced2, &tokens2);
            if (status2 != status || produced2 != produced || tokens2 != tokens || crc32_of(out2, produced2) != h) {
                std::fprintf(stderr, "stream %u: windowed decode at alignment %u gives %d %u %llu, the whole-stream decode %d %u %llu\n", i, m, status2, produced2,
                             (unsigned long long)tokens2, status, produced, (unsigned long long)tokens);
                differ = 3;
            }
            std::free(out2);
        }
        std::free(in);
        std::free(out);
    }
    std::free(S);
    std::fclose(f);
    return differ;
}
