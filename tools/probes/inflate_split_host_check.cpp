// inflate_split_host_check - the split decoder of raider_amd/csrc/inflate_kernels.h (rdr_inflate_decode_split) on the CPU: the candidate
// rule, the measure pass (infl_measure_run, what lane 0 of infl_measure_kernel runs), the plan (infl_plan, what the entry point runs on
// the host) and the pieces decoded one by one from an empty history, over zlib streams read from a file, for a build with
// -fsanitize=address,undefined:
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/probes/inflate_split_host_check.cpp -o inflate_split_host_check
//   ./inflate_split_host_check streams.bin
//
// streams.bin: as for inflate_host_check (u32 count, then per stream u32 input bytes, u32 output capacity, the input bytes).  Input and
// output live in heap blocks of exactly those sizes.  Prints one line per stream: status (RDR_INFL_*), bytes produced, CRC-32 of the
// output, pieces (1: the stream stayed whole).  No GPU call is made.
//
// Every stream is decoded twice into slots pre-filled with 0xA5: serially, as inflate_host_check does, and through scan / measure / plan /
// pieces, with the serial decode for a stream whose plan is not clean - the entry point's rule.  Status, produced and every byte of the
// two slots must agree.  Every piece is measured twice, with the whole stream as the window and through a staged window of INFL_WIN
// bytes at alignment (stream index mod 4); the two records must agree.  A difference is reported on stderr and the exit status is 3.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../raider_amd/csrc/inflate_kernels.h"

using namespace rdr;

static void apply(uint8_t* out, uint32_t o, int t) {
    if (t & INFL_TOK_MATCH) {
        const uint32_t len = (uint32_t)infl_tok_len(t), dist = (uint32_t)infl_tok_dist(t);
        for (uint32_t k = 0; k < len; ++k) out[o + k] = out[o + k - dist];
    } else
        out[o] = (uint8_t)t;
}

static void adler_of(const uint8_t* p, uint32_t n, uint32_t& A, uint32_t& B) {
    for (uint32_t k = 0; k < n; ++k) { A = (A + p[k]) % 65521u; B = (B + A) % 65521u; }
}

// the whole stream, one token at a time
static int decode(InflShared& S, const uint8_t* in, uint32_t nbytes, uint8_t* out, uint32_t cap, uint32_t* produced_out) {
    const InflTables T = infl_tables(S);
    const InflIn win{in, 0u, nbytes, nbytes};
    InflState st;
    inflate_init(st, 0u);
    uint32_t o = 0;
    int result = -1;
    while (result < 0) {
        const int t = inflate_next(win, st, T, o);
        if (t >= 0) {
            if ((uint32_t)infl_tok_len(t) > cap - o) { result = INFL_OVERFLOW; break; }
            apply(out, o, t);
            o += (uint32_t)infl_tok_len(t);
        } else if (t == INFL_EV_STORED) {
            if (st.stored_len > cap - o) { result = INFL_OVERFLOW; break; }
            if (st.stored_len) std::memcpy(out + o, in + st.b.pos, st.stored_len);
            o += st.stored_len;
            inflate_stored_done(st);
        } else if (t == INFL_EV_DONE) {
            uint32_t A = 1u, B = 0u;
            adler_of(out, o, A, B);
            result = ((B << 16) | A) == st.adler ? INFL_OK : INFL_CHECKSUM;
        } else if (t == INFL_EV_MORE)
            result = INFL_INVALID;                         // (cannot happen)
        else
            result = infl_status_of(t);
    }
    *produced_out = o;
    return result;
}

// the candidate rule of infl_scan_kernel: the first marker of every window of INFL_GAP bytes, and the complement of the last
static std::vector<uint32_t> scan(const uint8_t* in, uint32_t nbytes) {
    std::vector<uint32_t> cand(infl_slots(nbytes) - 1u, 0xffffffffu);
    for (uint64_t p = 6; p + 6 <= (uint64_t)nbytes; ++p)
        if (in[p - 4] == 0u && in[p - 3] == 0u && in[p - 2] == 0xffu && in[p - 1] == 0xffu) {
            uint32_t& c = cand[(size_t)(2 * (p / INFL_GAP))];
            uint32_t& d = cand[(size_t)(2 * (p / INFL_GAP) + 1)];
            if ((uint32_t)p < c) c = (uint32_t)p;
            if (~(uint32_t)p < d) d = ~(uint32_t)p;
        }
    return cand;
}

// one piece measured the way the kernel does it: m the alignment, a staged window (whole == false) or the stream itself
static InflPiece measure(InflShared& S, const uint8_t* in, uint32_t nbytes, uint32_t cap, const std::vector<uint32_t>& cand, uint32_t start, bool is_start, uint32_t m,
                         bool whole) {
    const InflTables T = infl_tables(S);
    uint8_t* stage = (uint8_t*)std::malloc(INFL_WIN);
    InflIn win{whole ? in : stage, 0u, whole ? nbytes : 0u, m + nbytes};
    InflState st;
    inflate_init(st, m);
    if (!is_start) { st.b.pos = m + start; st.mode = 1; }
    InflPiece P{start, 0u, 0u, 0u, 0u, INFL_P_BAD};
    uint64_t guard = 16ull * nbytes + 64ull;
    for (;;) {
        if (!whole) {
            infl_window(win, st.b.pos);
            for (uint32_t i = 0; i < (uint32_t)INFL_WIN; ++i) {
                const int64_t p = (int64_t)win.base + i - (int64_t)m;
                stage[i] = (p >= 0 && p < (int64_t)nbytes) ? in[p] : (uint8_t)0;
            }
        }
        if (guard-- == 0) { P.status = INFL_P_BAD; break; }
        if (!infl_measure_run(win, st, T, m, cap, cand.data(), (uint32_t)cand.size(), P)) break;
        if (whole) { P.status = INFL_P_BAD; break; }       // (cannot happen: nothing to stage)
    }
    std::free(stage);
    return P;
}

// one job from an empty history: what inflate_piece_kernel does with a ring
static void decode_piece(InflShared& S, const uint8_t* in, uint32_t nbytes, uint8_t* out, const InflJob& J, InflJobOut& R) {
    const InflTables T = infl_tables(S);
    const InflIn win{in, 0u, nbytes, nbytes};
    InflState st;
    inflate_init(st, 0u);
    if (J.pos) { st.b.pos = J.pos; st.mode = 1; }
    const uint32_t cap = J.out + J.len;
    uint32_t o = J.out, adler = 0u;
    int result = -1;
    while (result < 0) {
        const int t = inflate_next(win, st, T, o);
        if (t >= 0) {
            if ((uint32_t)infl_tok_len(t) > cap - o) { result = INFL_OVERFLOW; break; }
            apply(out, o, t);
            o += (uint32_t)infl_tok_len(t);
        } else if (t == INFL_EV_STORED) {
            if (st.stored_len > cap - o) { result = INFL_OVERFLOW; break; }
            if (st.stored_len) std::memcpy(out + o, in + st.b.pos, st.stored_len);
            o += st.stored_len;
            inflate_stored_done(st);
            if (st.b.pos == J.end) result = INFL_OK;
        } else if (t == INFL_EV_DONE) {
            adler = st.adler;
            result = INFL_OK;
        } else
            result = INFL_INVALID;
    }
    R = InflJobOut{1u, 0u, o - J.out, result};
    adler_of(out + J.out, R.len, R.A, R.B);
    if (R.len != J.len || (J.last && adler != J.adler)) R.status = INFL_INVALID;
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
        const uint32_t nbytes = hdr[0], cap = hdr[1];
        uint8_t* in = (uint8_t*)std::malloc(nbytes ? nbytes : 1);
        uint8_t* serial = (uint8_t*)std::malloc(cap ? cap : 1);
        uint8_t* split = (uint8_t*)std::malloc(cap ? cap : 1);
        if (nbytes && std::fread(in, 1, nbytes, f) != nbytes) return 2;
        std::memset(serial, 0xa5, cap ? cap : 1);
        std::memset(split, 0xa5, cap ? cap : 1);
        uint32_t produced = 0;
        const int status = decode(*S, in, nbytes, serial, cap, &produced);

        // scan, measure, plan
        const std::vector<uint32_t> cand = scan(in, nbytes);
        const uint32_t nslots = infl_slots(nbytes);
        std::vector<InflPiece> rec(nslots);
        std::memset(rec.data(), 0xff, nslots * sizeof(InflPiece));
        bool any = false;
        for (uint32_t c : cand) any = any || c != 0xffffffffu;
        uint32_t njobs = 0;
        std::vector<InflJob> jobs(nslots);
        if (any) {
            for (uint32_t j = 0; j < nslots; ++j) {
                const uint32_t start = j ? infl_candidate(cand.data(), j - 1u) : 0u;
                if (start == 0xffffffffu) continue;
                rec[j] = measure(*S, in, nbytes, cap, cand, start, j == 0, 0u, true);
                const InflPiece w = measure(*S, in, nbytes, cap, cand, start, j == 0, i & 3u, false);
                const InflPiece& r = rec[j];
                if (w.status != r.status || (r.status != INFL_P_BAD && (w.end != r.end || w.produced != r.produced || w.reach != r.reach || w.adler != r.adler))) {
                    std::fprintf(stderr, "stream %u: the piece at %u measures %d %u %u %u through a staged window, %d %u %u %u through the stream\n", i, start, w.status,
                                 w.end, w.produced, w.reach, r.status, r.end, r.produced, r.reach);
                    differ = 3;
                }
            }
            njobs = infl_plan(rec.data(), nslots, cap, (int32_t)i, jobs.data());
            if (njobs < 2) njobs = 0;
        }
        int status2 = status;
        uint32_t produced2 = produced;
        if (njobs) {                                               // the pieces, last to first: none may need what another one writes
            std::vector<InflJobOut> res(njobs);
            for (uint32_t k = njobs; k-- > 0;) decode_piece(*S, in, nbytes, split, jobs[k], res[k]);
            uint32_t A = 1u, B = 0u;
            bool ok = true;
            produced2 = 0;
            for (uint32_t k = 0; k < njobs; ++k) {
                ok = ok && res[k].status == INFL_OK;
                infl_adler_fold(A, B, res[k].A, res[k].B, res[k].len);
                produced2 += res[k].len;
            }
            status2 = !ok ? INFL_INVALID : ((B << 16) | A) == jobs[njobs - 1].adler ? INFL_OK : INFL_CHECKSUM;
        } else
            status2 = decode(*S, in, nbytes, split, cap, &produced2);
        if (status2 != status || produced2 != produced || std::memcmp(serial, split, cap) != 0) {
            std::fprintf(stderr, "stream %u: %u pieces give %d %u, the serial decode %d %u%s\n", i, njobs, status2, produced2, status, produced,
                         std::memcmp(serial, split, cap) != 0 ? ", and the slots differ" : "");
            differ = 3;
        }
        std::printf("%d %u %08x %u\n", status2, produced2, crc32_of(split, produced2), njobs ? njobs : 1u);
        std::free(in);
        std::free(serial);
        std::free(split);
    }
    std::free(S);
    std::fclose(f);
    return differ;
}
