// deflate_dynamic_host_check - the dynamic-table mode of raider_amd/csrc/deflate_kernels.h on the CPU, 64 threads standing in for the
// 64 lanes and a barrier for every wave operation (as deflate_host_check.cpp does for the fixed mode), for a build with sanitizers:
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined tools/probes/deflate_dynamic_host_check.cpp -o deflate_dynamic_host_check
//   ./deflate_dynamic_host_check streams in.bin out.bin
//   ./deflate_dynamic_host_check codes in.bin out.bin
//
// streams: in.bin is u32 count, then per stream u32 bytes and the bytes; out.bin is per stream u32 bytes and the zlib stream, put
// together from the sub-blocks of deflate_subblock_dyn() exactly as rdr_deflate_encode_tables + deflate_pack_kernel do.  One line per
// stream on stdout: "stream i: n -> z bytes, blocks: s f d ..." (the kind of every sub-block: stored, fixed, dynamic).  Input, slots and
// the token scratch live in heap blocks of exactly their sizes, so an access outside them is a sanitizer report.
// codes: in.bin is a sequence of histograms - u32 alphabet size (2 .. 286), u32 limit (<= 15, 2^limit >= size), then the u32 counts;
// out.bin is, per histogram, the u32 code lengths defl_build_lengths() gives them: the function every wave runs.
#include <pthread.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define RDR_DEFLATE_HOST_EMU 1
static pthread_barrier_t g_bar;
static uint32_t g_x[64];
static inline void wv_sync() { pthread_barrier_wait(&g_bar); }
static inline uint32_t wv_shfl(int lane, uint32_t v, int src) { g_x[lane] = v; wv_sync(); const uint32_t r = g_x[src & 63]; wv_sync(); return r; }
static inline uint32_t wv_shfl_up(int lane, uint32_t v, int d) { g_x[lane] = v; wv_sync(); const uint32_t r = lane >= d ? g_x[lane - d] : v; wv_sync(); return r; }
static inline uint64_t wv_ballot(int lane, bool p) {
    g_x[lane] = p; wv_sync();
    uint64_t m = 0; for (int i = 0; i < 64; ++i) m |= (uint64_t)(g_x[i] & 1u) << i;
    wv_sync(); return m;
}
static inline void wv_atomic_max(uint32_t* p, uint32_t v) { uint32_t o = __atomic_load_n(p, __ATOMIC_RELAXED); while (o < v && !__atomic_compare_exchange_n(p, &o, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {} }
static inline void wv_atomic_or(uint32_t* p, uint32_t v) { __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
static inline void wv_atomic_add(uint32_t* p, uint32_t v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

#include "../../raider_amd/csrc/deflate_kernels.h"

using namespace rdr;

struct Job { const uint8_t* src; int n; bool last; uint32_t* slot; DeflResult res; };
struct Hist { std::vector<uint32_t> cnt, lens; int limit; uint32_t* work; };
static std::vector<Job> g_jobs;
static std::vector<Hist> g_hists;
static DeflShared* g_S;
static uint32_t* g_tok;

static void* lane_main(void* arg) {
    const int lane = (int)(intptr_t)arg;
    for (auto& j : g_jobs) {
        const DeflResult r = deflate_subblock_dyn(lane, *g_S, j.src, j.n, j.last, j.slot, g_tok);
        if (lane == 0) j.res = r;
        wv_sync();
    }
    for (auto& h : g_hists) defl_build_lengths(lane, h.cnt.data(), (int)h.cnt.size(), h.limit, h.lens.data(), h.work);
    return nullptr;
}

static void run_lanes() {
    pthread_barrier_init(&g_bar, nullptr, 64);
    pthread_t th[64];
    for (int i = 0; i < 64; ++i) pthread_create(&th[i], nullptr, lane_main, (void*)(intptr_t)i);
    for (int i = 0; i < 64; ++i) pthread_join(th[i], nullptr);
}

static int codes(FILE* f, const char* out_path) {
    uint32_t hd[2];
    while (std::fread(hd, 4, 2, f) == 2) {
        if (hd[0] < 2 || hd[0] > (uint32_t)DEFL_NLL || hd[1] < 1 || hd[1] > 15 || (1u << hd[1]) < hd[0]) { std::fprintf(stderr, "bad histogram header %u %u\n", hd[0], hd[1]); return 2; }
        Hist h{std::vector<uint32_t>(hd[0]), std::vector<uint32_t>(hd[0]), (int)hd[1], (uint32_t*)std::malloc(sizeof(uint32_t) * DEFL_PM_WORK)};
        if (std::fread(h.cnt.data(), 4, hd[0], f) != hd[0]) return 2;
        g_hists.push_back(std::move(h));
    }
    std::fclose(f);
    run_lanes();
    FILE* o = std::fopen(out_path, "wb");
    if (!o) { std::perror(out_path); return 2; }
    for (auto& h : g_hists) { std::fwrite(h.lens.data(), 4, h.lens.size(), o); std::free(h.work); }
    std::fclose(o);
    std::printf("%zu histograms\n", g_hists.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4 || (std::strcmp(argv[1], "streams") && std::strcmp(argv[1], "codes"))) { std::fprintf(stderr, "usage: %s streams|codes in.bin out.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) { std::perror(argv[2]); return 2; }
    if (!std::strcmp(argv[1], "codes")) return codes(f, argv[3]);
    uint32_t count = 0;
    if (std::fread(&count, 4, 1, f) != 1) return 2;
    std::vector<uint8_t*> bufs; std::vector<uint32_t> lens;
    std::vector<std::vector<size_t>> jobs_of(count);
    for (uint32_t s = 0; s < count; ++s) {
        uint32_t n = 0;
        if (std::fread(&n, 4, 1, f) != 1) return 2;
        const uint32_t shift = s % 4;                                   // every source alignment
        uint8_t* b = (uint8_t*)std::malloc(n + shift);
        if (n && std::fread(b + shift, 1, n, f) != n) return 2;
        bufs.push_back(b); lens.push_back(n);
        for (uint32_t o = 0; o < n; o += DEFL_SUB) {
            const int m = (int)(n - o < (uint32_t)DEFL_SUB ? n - o : (uint32_t)DEFL_SUB);
            jobs_of[s].push_back(g_jobs.size());
            g_jobs.push_back(Job{b + shift + o, m, o + m == n, (uint32_t*)std::malloc(DEFL_SLOT), DeflResult{}});
        }
    }
    std::fclose(f);
    g_S = new DeflShared;
    g_tok = (uint32_t*)std::malloc(sizeof(uint32_t) * DEFL_SUB);
    run_lanes();
    FILE* o = std::fopen(argv[3], "wb");
    if (!o) { std::perror(argv[3]); return 2; }
    for (uint32_t s = 0; s < count; ++s) {
        std::vector<uint8_t> z = {0x78, 0x01};
        uint32_t A = 1, B = 0;
        std::printf("stream %u: %u ->", s, lens[s]);
        std::vector<char> kinds;
        for (size_t k : jobs_of[s]) {
            const Job& j = g_jobs[k];
            B = (uint32_t)((B + (uint64_t)j.n % 65521u * A + j.res.s2) % 65521u);
            A = (A + j.res.s1) % 65521u;
            kinds.push_back(j.res.fixed_bytes > 0 ? (j.res.pad == 2 ? 'd' : 'f') : 's');
            if (j.res.fixed_bytes > 0) z.insert(z.end(), (const uint8_t*)j.slot, (const uint8_t*)j.slot + j.res.fixed_bytes);
            else {
                const uint8_t h[5] = {(uint8_t)(j.last ? 1 : 0), (uint8_t)(j.n & 0xff), (uint8_t)(j.n >> 8), (uint8_t)(~j.n & 0xff), (uint8_t)((~j.n >> 8) & 0xff)};
                z.insert(z.end(), h, h + 5); z.insert(z.end(), j.src, j.src + j.n);
            }
        }
        const uint32_t ad = (B << 16) | A;
        const uint8_t t[4] = {(uint8_t)(ad >> 24), (uint8_t)(ad >> 16), (uint8_t)(ad >> 8), (uint8_t)ad};
        z.insert(z.end(), t, t + 4);
        const uint32_t zn = (uint32_t)z.size();
        std::fwrite(&zn, 4, 1, o); std::fwrite(z.data(), 1, zn, o);
        std::printf(" %u bytes, blocks:", zn);
        for (char c : kinds) std::printf(" %c", c);
        std::printf("\n");
    }
    std::fclose(o);
    for (auto& j : g_jobs) std::free(j.slot);
    for (auto* b : bufs) std::free(b);
    std::free(g_tok);
    delete g_S;
    return 0;
}
