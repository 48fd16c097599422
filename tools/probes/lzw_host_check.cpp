// lzw_host_check - the LZW bit reader, table update and string expansion of raider_amd/csrc/tiff_kernels.h (the __host__ __device__
// functions the device kernel runs) on the CPU, over streams read from a file, for a build with -fsanitize=address,undefined:
//
//   hipcc --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined tools/probes/lzw_host_check.cpp -o lzw_host_check
//   ./lzw_host_check streams.bin
//
// streams.bin: u32 count, then per stream u32 input bytes, u32 output capacity, the input bytes (little-endian).  Input and output live
// in heap blocks of exactly those sizes, so any access outside a stream's own bytes is a sanitizer report.  Prints one line per
// stream: status (0 ok, 1 short, 2 bad code), bytes produced, FNV-1a of the output.  No GPU call is made.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../raider_amd/csrc/tiff_kernels.h"

using namespace rdr;

static int decode(const uint8_t* in, uint32_t nbytes, uint8_t* out, uint32_t cap, uint32_t* produced_out) {
    std::vector<uint16_t> prefix(LZW_TABLE), length(LZW_TABLE);
    std::vector<uint8_t> last(LZW_TABLE), first(LZW_TABLE);
    const LzwTable tab{prefix.data(), length.data(), last.data(), first.data()};
    lzw_table_init(tab, 0, 1);
    LzwState st{0, 0, 0, 9, LZW_FIRST, -1};
    uint32_t produced = 0;
    for (;;) {
        const int code = lzw_next(in, 0, nbytes, nbytes, st, tab);
        if (code == LZW_CLEARED) continue;
        if (code < 0) {
            *produced_out = produced;
            if (code == LZW_END_EOI) return LZW_OK;
            if (code == LZW_END_BAD) return LZW_BAD_CODE;
            return produced == cap ? LZW_OK : LZW_SHORT;          // LZW_END_INPUT (LZW_MORE_WINDOW cannot happen: the window is the stream)
        }
        const uint32_t len = length[code];
        const uint32_t take = len < cap - produced ? len : cap - produced;
        if (take) lzw_expand(tab, code, 0, (int)take, out, (int)produced);
        produced += take;
        if (take < len) { *produced_out = produced; return LZW_SHORT; }
    }
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s streams.bin\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    uint32_t n = 0;
    if (std::fread(&n, 4, 1, f) != 1) return 2;
    for (uint32_t i = 0; i < n; ++i) {
        uint32_t hdr[2];
        if (std::fread(hdr, 4, 2, f) != 2) return 2;
        uint8_t* in = (uint8_t*)std::malloc(hdr[0] ? hdr[0] : 1);
        uint8_t* out = (uint8_t*)std::malloc(hdr[1] ? hdr[1] : 1);
        if (hdr[0] && std::fread(in, 1, hdr[0], f) != hdr[0]) return 2;
        std::memset(out, 0, hdr[1] ? hdr[1] : 1);
        uint32_t produced = 0;
        const int status = decode(in, hdr[0], out, hdr[1], &produced);
        uint64_t h = 1469598103934665603ull;
        for (uint32_t k = 0; k < produced; ++k) { h ^= out[k]; h *= 1099511628211ull; }
        std::printf("%d %u %016llx\n", status, produced, (unsigned long long)h);
        std::free(in);
        std::free(out);
    }
    std::fclose(f);
    return 0;
}
