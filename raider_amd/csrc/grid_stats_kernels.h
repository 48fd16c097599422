// Gridded station statistics of raiderStats (cli/statsPlot.py create_DF, :1571-1794): per station and per grid cell the count, mean,
// median and standard deviation (ddof = 1) of a [nd][n] station series with NaN = no row, the stations sorted by cell.  Included by
// raider_hip.hip after cell_variogram_kernels.h, whose cv_reduce (a workgroup sum in a fixed order) is reused.
//
// Means and deviations: two passes, the mean and then the centred squares, f64, every sum in a fixed order (per lane in the order of
// its loads, lanes by shuffles, waves in order), so two calls give the same bytes.  No floating-point atomic anywhere.
//
// Medians: exact selection.  A double that is not NaN maps to its order-preserving 64-bit key (sign bit flipped for positives, all
// bits for negatives: -inf < ... < -0 < +0 < ... < +inf).  Eight passes, from the top byte down, each counting the byte of the keys
// that share the prefix found so far into 256 bins and picking the bin that holds rank (m - 1) / 2; after the eighth the prefix IS the
// key of that rank (lo).  One further pass counts the keys <= lo and finds the smallest key above it: the element of rank m / 2 (hi)
// is lo again when at least m / 2 + 1 keys are <= lo, else that successor.  median = (lo + hi) / 2 - for sorted valid values s,
// (s[(m - 1) / 2] + s[m / 2]) / 2, what pandas computes.
//
// Two shapes of segment, two kernels:
//   grid_stats_station_kernel  a workgroup of four waves owns 64 neighbouring stations, lane l of every wave station l of them: a row
//                              of values is read by consecutive lanes (coalesced), wave w reads the dates w, w + 4, ...  The lanes'
//                              histograms live in LDS, bin b of lane l in half (b & 1) of the dword (b >> 1) * 64 + l: every lane in
//                              its own bank, two 16-bit counters per dword (a bin holds at most nd <= 4096), the four waves adding
//                              through integer LDS atomics.  32 KiB + 5 KiB of reduction rows.
//   grid_stats_cell_kernel     a workgroup owns one cell: its lanes stride over the linear index of the slab nd x m (date-major, the
//                              (date, station) of a lane advanced incrementally, without a division per element), one 256-bin
//                              histogram of 32-bit counters in LDS, filled by integer atomics; a slab holds at most 2^31 - 1 slots.
//                              Then the means of the cell's station statistics, each summed by one lane in station order.
// A huge cell runs in one workgroup, as in rdr_cell_variogram: no speed is promised there.
#pragma once

constexpr int GS_TILE = 256;                  // lanes of a workgroup (= VG_TILE: cv_reduce is shared)
constexpr int GS_WAVES = GS_TILE / 64;
constexpr int GS_STATIONS = 64;               // stations of a workgroup of the station kernel
static_assert(GS_TILE == VG_TILE && GS_WAVES == VG_WAVES, "cv_reduce adds the four waves of a 256-lane workgroup");

struct GridStatsArgs {
    const double* values; const long long* cell_start; long long n; int nd;
    long long* st_nobs; double *st_mean, *st_median, *st_stdev;                       // st_median NULL: no station medians
    long long* nstations; double *mean_of_means, *mean_of_medians, *mean_of_stdevs;   // nstations NULL: the group is skipped
    long long* cell_nobs; double *abs_mean, *abs_median, *abs_stdev;                  // cell_nobs NULL: the group is skipped
};

__device__ __forceinline__ unsigned long long gs_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double gs_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

// (lo + hi) / 2 of the two middle keys; hi is lo itself for an odd count or when the keys <= lo reach past rank m / 2
__device__ __forceinline__ double gs_median_of(unsigned int m, unsigned long long lo_key, unsigned int n_le, unsigned long long above) {
#pragma clang fp contract(off)
    const double lo = gs_unkey(lo_key);
    const double hi = ((m & 1u) || n_le >= m / 2u + 1u) ? lo : gs_unkey(above);
    return (lo + hi) / 2.0;
}

// ---- per station ---------------------------------------------------------------------------------------------------------------------
struct GsStationShared {
    unsigned int hist[128 * GS_STATIONS];
    double dsum[GS_WAVES][GS_STATIONS];
    unsigned long long umin[GS_WAVES][GS_STATIONS];
    unsigned int cnt[GS_WAVES][GS_STATIONS];
};

// the dates wave, wave + 4, ... of one station's column, in that order, four loads in flight; a lane without a station sees NaN only
template <typename F>
__device__ __forceinline__ void gs_column(const double* col, size_t n, int nd, int wave, bool live, F&& f) {
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    int d = wave;
    for (; d + 3 * GS_WAVES < nd; d += 4 * GS_WAVES) {
        double v0 = qnan, v1 = qnan, v2 = qnan, v3 = qnan;
        if (live) {
            v0 = col[(size_t)d * n]; v1 = col[(size_t)(d + GS_WAVES) * n];
            v2 = col[(size_t)(d + 2 * GS_WAVES) * n]; v3 = col[(size_t)(d + 3 * GS_WAVES) * n];
        }
        f(v0); f(v1); f(v2); f(v3);
    }
    for (; d < nd; d += GS_WAVES) f(live ? col[(size_t)d * n] : qnan);
}

__global__ __launch_bounds__(GS_TILE) void grid_stats_station_kernel(GridStatsArgs A) {
    __shared__ GsStationShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const long long s = (long long)blockIdx.x * GS_STATIONS + lane;
    const bool live = s < A.n;
    const double* col = A.values + (live ? s : 0);
    const size_t n = (size_t)A.n;
    const int nd = A.nd;

    // the count and the mean
    double sum = 0.0; unsigned int c = 0u;
    gs_column(col, n, nd, wave, live, [&](double v) { if (v == v) { sum += v; ++c; } });
    S.dsum[wave][lane] = sum; S.cnt[wave][lane] = c;
    __syncthreads();
    const unsigned int m = ((S.cnt[0][lane] + S.cnt[1][lane]) + S.cnt[2][lane]) + S.cnt[3][lane];
    const double mean = m ? (((S.dsum[0][lane] + S.dsum[1][lane]) + S.dsum[2][lane]) + S.dsum[3][lane]) / (double)m : qnan;
    __syncthreads();
    // the centred squares
    double ss = 0.0;
    gs_column(col, n, nd, wave, live, [&](double v) { if (v == v) { const double dv = v - mean; ss += dv * dv; } });
    S.dsum[wave][lane] = ss;
    __syncthreads();
    const double sst = ((S.dsum[0][lane] + S.dsum[1][lane]) + S.dsum[2][lane]) + S.dsum[3][lane];
    if (wave == 0 && live) {
        A.st_nobs[s] = (long long)m;
        A.st_mean[s] = mean;
        A.st_stdev[s] = m >= 2u ? sqrt(sst / (double)(m - 1u)) : qnan;
    }
    if (!A.st_median) return;                 // (the same in every lane)

    // the key of rank (m - 1) / 2, a byte per pass
    unsigned long long prefix = 0ull;
    unsigned int r = m ? (m - 1u) / 2u : 0u;
    for (int p = 7; p >= 0; --p) {
        __syncthreads();                      // (the last pass's bins and the reduction rows have been read)
        for (int k = tid; k < 128 * GS_STATIONS; k += GS_TILE) S.hist[k] = 0u;
        __syncthreads();
        const int sh = 8 * p;
        gs_column(col, n, nd, wave, live, [&](double v) {
            if (v == v) {
                const unsigned long long key = gs_key(v);
                if (p == 7 || ((key >> sh) >> 8) == prefix) {
                    const unsigned int b = (unsigned int)(key >> sh) & 255u;
                    atomicAdd(&S.hist[(b >> 1) * GS_STATIONS + lane], 1u << ((b & 1u) * 16u));
                }
            }
        });
        __syncthreads();
        unsigned int cum = 0u, bin = 0u; bool found = false;
        for (unsigned int w2 = 0; w2 < 128u; ++w2) {
            const unsigned int w = S.hist[w2 * GS_STATIONS + lane], c0 = w & 0xffffu, c1 = w >> 16;
            if (!found) {
                if (cum + c0 > r) { found = true; bin = 2u * w2; r -= cum; }
                else if (cum + c0 + c1 > r) { found = true; bin = 2u * w2 + 1u; r -= cum + c0; }
                else cum += c0 + c1;
            }
        }
        prefix = (prefix << 8) | bin;
    }
    // its successor: the keys <= it, and the smallest key above it
    unsigned int n_le = 0u; unsigned long long above = ~0ull;
    gs_column(col, n, nd, wave, live, [&](double v) {
        if (v == v) {
            const unsigned long long key = gs_key(v);
            if (key <= prefix) ++n_le; else if (key < above) above = key;
        }
    });
    S.cnt[wave][lane] = n_le; S.umin[wave][lane] = above;
    __syncthreads();
    if (wave == 0 && live) {
        unsigned int le = 0u; unsigned long long ab = ~0ull;
#pragma unroll
        for (int w = 0; w < GS_WAVES; ++w) { le += S.cnt[w][lane]; const unsigned long long t = S.umin[w][lane]; ab = t < ab ? t : ab; }
        A.st_median[s] = m ? gs_median_of(m, prefix, le, ab) : qnan;
    }
}

// ---- per cell ------------------------------------------------------------------------------------------------------------------------
struct GsCellShared {
    unsigned int hist[256];
    double red[GS_WAVES];
    unsigned int cnt;
    unsigned long long above;
};

// the workgroup's lanes over the slab nd x m (m >= 1) in the order of the linear index q = date * m + station: q = tid, tid + 256, ...
template <typename F>
__device__ __forceinline__ void gs_slab(const double* base, size_t n, int nd, int m, F&& f) {
    const int qd = GS_TILE / m, qr = GS_TILE % m;
    auto step = [&](int& d, int& k) { d += qd; k += qr; if (k >= m) { k -= m; ++d; } };
    int d = (int)threadIdx.x / m, k = (int)threadIdx.x % m;
    for (;;) {                                // four loads in flight while four steps stay inside the slab (d never decreases)
        int d1 = d, k1 = k; step(d1, k1);
        int d2 = d1, k2 = k1; step(d2, k2);
        int d3 = d2, k3 = k2; step(d3, k3);
        if (d3 >= nd) break;
        const double v0 = base[(size_t)d * n + k], v1 = base[(size_t)d1 * n + k1], v2 = base[(size_t)d2 * n + k2], v3 = base[(size_t)d3 * n + k3];
        f(v0); f(v1); f(v2); f(v3);
        d = d3; k = k3; step(d, k);
    }
    while (d < nd) {
        f(base[(size_t)d * n + k]);
        step(d, k);
    }
}

// v <- its sum over the workgroup, in every lane (integer: any order gives the same)
__device__ __forceinline__ unsigned int gs_count(unsigned int v, unsigned int* cell) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (threadIdx.x == 0) *cell = 0u;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) atomicAdd(cell, v);
    __syncthreads();
    const unsigned int t = *cell;
    __syncthreads();                          // (the cell may be written again)
    return t;
}

// the mean of src[0 .. m) without its NaNs, added in index order by the calling lane; NaN when nothing is left
__device__ __forceinline__ double gs_mean_of(const double* src, int m) {
    double sum = 0.0; long long k = 0;
    for (int i = 0; i < m; ++i) { const double v = src[i]; if (v == v) { sum += v; ++k; } }
    return k ? sum / (double)k : __longlong_as_double(0x7ff8000000000000ll);
}

__global__ __launch_bounds__(GS_TILE) void grid_stats_cell_kernel(GridStatsArgs A) {
    __shared__ GsCellShared S;
    const int tid = threadIdx.x, cell = blockIdx.x;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const long long s0 = A.cell_start[cell];
    const int m = (int)(A.cell_start[cell + 1] - s0);
    const int nd = A.nd;
    const size_t n = (size_t)A.n;

    if (A.nstations) {                        // the station kernel has finished: this launch follows it on the stream
        if (tid == 0) {
            long long ns = 0;
            for (int i = 0; i < m; ++i) ns += A.st_nobs[s0 + i] > 0 ? 1 : 0;
            A.nstations[cell] = ns;
        } else if (tid == 64) {
            A.mean_of_means[cell] = gs_mean_of(A.st_mean + s0, m);
        } else if (tid == 128) {
            A.mean_of_stdevs[cell] = gs_mean_of(A.st_stdev + s0, m);
        } else if (tid == 192 && A.mean_of_medians) {
            A.mean_of_medians[cell] = gs_mean_of(A.st_median + s0, m);
        }
    }
    if (!A.cell_nobs) return;
    if (m == 0) {
        if (tid == 0) {
            A.cell_nobs[cell] = 0; A.abs_mean[cell] = qnan; A.abs_stdev[cell] = qnan;
            if (A.abs_median) A.abs_median[cell] = qnan;
        }
        return;
    }
    const double* base = A.values + s0;

    unsigned int c = 0u; double a[1] = {0.0};
    gs_slab(base, n, nd, m, [&](double v) { if (v == v) { a[0] += v; ++c; } });
    const unsigned int cnt = gs_count(c, &S.cnt);
    cv_reduce<1>(a, S.red);
    const double mean = cnt ? a[0] / (double)cnt : qnan;
    a[0] = 0.0;
    gs_slab(base, n, nd, m, [&](double v) { if (v == v) { const double dv = v - mean; a[0] += dv * dv; } });
    cv_reduce<1>(a, S.red);
    if (tid == 0) {
        A.cell_nobs[cell] = (long long)cnt;
        A.abs_mean[cell] = mean;
        A.abs_stdev[cell] = cnt >= 2u ? sqrt(a[0] / (double)(cnt - 1u)) : qnan;
    }
    if (!A.abs_median) return;
    if (cnt == 0u) { if (tid == 0) A.abs_median[cell] = qnan; return; }      // (cnt is the same in every lane)

    unsigned long long prefix = 0ull;
    unsigned int r = (cnt - 1u) / 2u;
    for (int p = 7; p >= 0; --p) {
        S.hist[tid] = 0u;                     // (GS_TILE = 256 bins; the last pass's bins were read before its closing barrier)
        __syncthreads();
        const int sh = 8 * p;
        gs_slab(base, n, nd, m, [&](double v) {
            if (v == v) {
                const unsigned long long key = gs_key(v);
                if (p == 7 || ((key >> sh) >> 8) == prefix) atomicAdd(&S.hist[(unsigned int)(key >> sh) & 255u], 1u);
            }
        });
        __syncthreads();
        unsigned int cum = 0u, bin = 0u; bool found = false;      // every lane walks the same bins (broadcast reads)
        for (unsigned int b = 0; b < 256u; ++b) {
            const unsigned int h = S.hist[b];
            if (!found) {
                if (cum + h > r) { found = true; bin = b; r -= cum; } else cum += h;
            }
        }
        prefix = (prefix << 8) | bin;
        __syncthreads();
    }
    unsigned int n_le = 0u; unsigned long long above = ~0ull;
    gs_slab(base, n, nd, m, [&](double v) {
        if (v == v) {
            const unsigned long long key = gs_key(v);
            if (key <= prefix) ++n_le; else if (key < above) above = key;
        }
    });
    if (tid == 0) S.above = ~0ull;
    const unsigned int le = gs_count(n_le, &S.cnt);               // (its first barrier also publishes S.above)
    for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(above, o, 64); above = t < above ? t : above; }
    if ((tid & 63) == 0) atomicMin(&S.above, above);
    __syncthreads();
    if (tid == 0) A.abs_median[cell] = gs_median_of(cnt, prefix, le, S.above);
}
