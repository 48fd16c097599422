// deflate_host_check - deflate_subblock() of raider_amd/csrc/deflate_kernels.h (the function every wave of deflate_encode_kernel runs)
// on the CPU, 64 threads standing in for the 64 lanes and a barrier for every wave operation, for a build with sanitizers:
//
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined tools/probes/deflate_host_check.cpp -o deflate_host_check
//   ./deflate_host_check streams_in.bin streams_out.bin
//
// streams_in.bin: u32 count, then per stream u32 bytes and the bytes.  streams_out.bin: per stream u32 bytes and the zlib stream, put
// together from the sub-blocks exactly as rdr_deflate_encode + deflate_pack_kernel do.  Input and slots live in heap blocks of exactly
// their sizes, so an access outside them is a sanitizer report.  The streams are then checked by zlib.decompress (tests or a few
// lines of Python); no GPU call is made.
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

#include "../../raider_amd/csrc/deflate_kernels.h"

using namespace rdr;

struct Job { const uint8_t* src; int n; bool last; uint32_t* slot; DeflResult res; };
static std::vector<Job> g_jobs;
static DeflShared* g_S;

static void* lane_main(void* arg) {
    const int lane = (int)(intptr_t)arg;
    for (auto& j : g_jobs) {
        const DeflResult r = deflate_subblock(lane, *g_S, j.src, j.n, j.last, j.slot);
        if (lane == 0) j.res = r;
        wv_sync();
    }
    return nullptr;
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
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
    pthread_barrier_init(&g_bar, nullptr, 64);
    pthread_t th[64];
    for (int i = 0; i < 64; ++i) pthread_create(&th[i], nullptr, lane_main, (void*)(intptr_t)i);
    for (int i = 0; i < 64; ++i) pthread_join(th[i], nullptr);
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    for (uint32_t s = 0; s < count; ++s) {
        std::vector<uint8_t> z = {0x78, 0x01};
        uint32_t A = 1, B = 0;
        for (size_t k : jobs_of[s]) {
            const Job& j = g_jobs[k];
            B = (uint32_t)((B + (uint64_t)j.n % 65521u * A + j.res.s2) % 65521u);
            A = (A + j.res.s1) % 65521u;
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
        std::printf("stream %u: %u -> %u bytes\n", s, lens[s], zn);
    }
    std::fclose(o);
    for (auto& j : g_jobs) std::free(j.slot);
    for (auto* b : bufs) std::free(b);
    delete g_S;
    return 0;
}
