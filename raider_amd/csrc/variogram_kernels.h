// Exact all-pair empirical variograms of a station series (cli/statsPlot.py:573-659, VariogramAnalysis), included by raider_hip.hip.
//
// N stations (x, y in metres), D dates of values v[d][i] (NaN = missing).  Every pair i < j gives h = sqrt(dx*dx + dy*dy) - without
// contraction, the value NumPy gets - and, on every date on which both values are there, g = 0.5 * (v_i - v_j)^2; the pair goes to the
// bin b with edges[b] < h <= edges[b + 1] (the rule of _binned_vario, :644), where count, sum of h and sum of g are kept.
//
// Work layout.  The upper triangle of the pair matrix is cut into tiles of VG_TILE x VG_TILE; a workgroup of VG_TILE lanes takes tile
// pairs (I <= J) p = blockIdx.x, + gridDim.x, ...  A lane owns ONE i of tile I - its x, y and the G <= 4 values of the launch's dates
// stay in registers - and walks the j of tile J, which sits in LDS (every lane reads the same j: a broadcast).  The distance of a pair
// is computed once for the G dates of a launch; further date groups recompute it (engine.epoch_groups' idiom).  The bin is found by a
// branch-free binary search of h in the edge row(s) kept in LDS, padded with +inf to 128 entries.  Accumulators are LDS histograms, one
// per wave, merged per workgroup at the end: each workgroup writes ONE partial [G][nbins] block, and pair_reduce_kernel adds the
// partials in workgroup order.  No floating-point atomic touches global memory; sums are f64 throughout.
#pragma once

constexpr int VG_TILE = 256;          // lanes of a workgroup = points of a tile (raider_amd/variogram.py: TILE)
constexpr int VG_WAVES = VG_TILE / 64;
constexpr int VG_MAXB = 64;           // bins
constexpr int VG_EPAD = 128;          // edge row in LDS: up to 65 edges, +inf behind them (the search reads up to index 126)

// tile pair p of the upper triangle of nt x nt tiles, rows first: (I, J) with I <= J
__device__ __forceinline__ void vg_tile_pair(long long p, int nt, int& I, int& J) {
    const double b = 2.0 * nt + 1.0;
    int i = (int)((b - sqrt(b * b - 8.0 * (double)p)) * 0.5);
    i = max(0, min(i, nt - 1));
    // first(i) = i * nt - i * (i - 1) / 2: the index of (i, i)
    while (i > 0 && (long long)i * nt - (long long)i * (i - 1) / 2 > p) --i;
    while (i + 1 < nt && (long long)(i + 1) * nt - (long long)(i + 1) * i / 2 <= p) ++i;
    I = i;
    J = i + (int)(p - ((long long)i * nt - (long long)i * (i - 1) / 2));
}

template <int G> struct VgVals { double v[G]; };

// The pair walk of one workgroup, shared by the two kernels: stages tile J, calls f(h2 operands...) per pair
template <int G, typename F>
__device__ __forceinline__ void vg_walk(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ v, int n, int d0,
                                        double2* sxy, double* sv, F&& f) {
    const int nt = (n + VG_TILE - 1) / VG_TILE;
    const long long ntp = (long long)nt * (nt + 1) / 2;
    const int tid = threadIdx.x;
    for (long long p = blockIdx.x; p < ntp; p += gridDim.x) {
        int I, J;
        vg_tile_pair(p, nt, I, J);
        const int i = I * VG_TILE + tid, jg = J * VG_TILE + tid;
        const int nj = min(VG_TILE, n - J * VG_TILE);
        __syncthreads();                                  // the previous tile pair's readers are done
        if (jg < n) {
            sxy[tid] = make_double2(x[jg], y[jg]);
#pragma unroll
            for (int g = 0; g < G; ++g) sv[tid * G + g] = v[(size_t)(d0 + g) * n + jg];
        }
        __syncthreads();
        if (i >= n) continue;                             // (no barrier below in this iteration)
        const double xi = x[i], yi = y[i];
        VgVals<G> vi;
#pragma unroll
        for (int g = 0; g < G; ++g) vi.v[g] = v[(size_t)(d0 + g) * n + i];
        const int j0 = I == J ? tid + 1 : 0;              // the diagonal tile: j > i only
        for (int j = j0; j < nj; ++j) {
            const double2 pj = sxy[j];
            f(xi - pj.x, yi - pj.y, vi, &sv[j * G]);
        }
    }
}

// squared distance as NumPy's dx*dx + dy*dy: two rounded products, one rounded sum
__device__ __forceinline__ double vg_dist2(double dx, double dy) {
#pragma clang fp contract(off)
    const double a = dx * dx, b = dy * dy;
    return a + b;
}

// hmax2[d0 + g] (unsigned 64-bit words, zeroed by the host): 1 + the bit pattern of the largest dx*dx + dy*dy over the pairs valid on
// the date - of non-negative doubles the patterns order as the numbers do, so an INTEGER atomic max merges the workgroups; 0 = no pair
template <int G>
__global__ __launch_bounds__(VG_TILE) void pair_hmax_kernel(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ v,
                                                            int n, int d0, unsigned long long* __restrict__ hmax2) {
    __shared__ double2 sxy[VG_TILE];
    __shared__ double sv[VG_TILE * G];
    __shared__ unsigned long long sm[G];
    if (threadIdx.x < G) sm[threadIdx.x] = 0ull;
    unsigned long long m[G];
#pragma unroll
    for (int g = 0; g < G; ++g) m[g] = 0ull;
    vg_walk<G>(x, y, v, n, d0, sxy, sv, [&](double dx, double dy, const VgVals<G>& vi, const double* vj) {
        const double d2 = vg_dist2(dx, dy);
        if (!(d2 >= 0.0)) return;                         // (a NaN coordinate: the pair is nobody's maximum, as for nanmax)
        const unsigned long long w = (unsigned long long)__double_as_longlong(d2) + 1ull;
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (vi.v[g] == vi.v[g] && vj[g] == vj[g] && w > m[g]) m[g] = w;
    });
#pragma unroll
    for (int g = 0; g < G; ++g) {
        unsigned long long w = m[g];
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(w, o, 64); w = t > w ? t : w; }
        m[g] = w;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int g = 0; g < G; ++g) if (m[g]) atomicMax(&sm[g], m[g]);
    __syncthreads();
    if (threadIdx.x < G && sm[threadIdx.x]) atomicMax(&hmax2[d0 + threadIdx.x], sm[threadIdx.x]);
}

// hmax[d] = sqrt of the largest squared distance (the square root is monotone: this IS the largest h); NaN without a valid pair
__global__ void pair_hmax_finish_kernel(const unsigned long long* __restrict__ hmax2, int nd, double* __restrict__ hmax) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= nd) return;
    const unsigned long long w = hmax2[d];
    hmax[d] = w ? sqrt(__longlong_as_double((long long)(w - 1ull))) : __longlong_as_double(0x7ff8000000000000ll);
}

// how many of the row's edges lie strictly below h (0 .. ne): e[] holds the ne edges and +inf up to VG_EPAD
__device__ __forceinline__ int vg_below(const double* e, double h) {
    int pos = 0;
#pragma unroll
    for (int s = 64; s > 0; s >>= 1) pos += (e[pos + s - 1] < h) ? s : 0;
    return pos;
}

// part_*: [gridDim.x][G * nbins] - the workgroup's sums over ITS tile pairs, every element written (an empty bin as 0)
template <int G>
__global__ __launch_bounds__(VG_TILE) void pair_variogram_kernel(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ v,
                                                                 int n, int d0, const double* __restrict__ edges, int per_date, int nbins,
                                                                 unsigned long long* __restrict__ part_count, double* __restrict__ part_lag,
                                                                 double* __restrict__ part_gamma) {
    __shared__ double2 sxy[VG_TILE];
    __shared__ double sv[VG_TILE * G];
    __shared__ double se[G * VG_EPAD];
    __shared__ double slag[VG_WAVES][G * VG_MAXB], sgam[VG_WAVES][G * VG_MAXB];
    __shared__ unsigned int scnt[VG_WAVES][G * VG_MAXB];
    const int tid = threadIdx.x, wave = tid >> 6;
    const int ne = nbins + 1, rows = per_date ? G : 1;
    for (int k = tid; k < rows * VG_EPAD; k += VG_TILE) {
        const int r = k / VG_EPAD, c = k % VG_EPAD;
        se[k] = c < ne ? edges[(size_t)(per_date ? d0 + r : 0) * ne + c] : __longlong_as_double(0x7ff0000000000000ll);
    }
    for (int k = tid; k < VG_WAVES * G * VG_MAXB; k += VG_TILE) { (&slag[0][0])[k] = 0.0; (&sgam[0][0])[k] = 0.0; (&scnt[0][0])[k] = 0u; }
    // (vg_walk's first barrier publishes the tables)
    double* wl = slag[wave]; double* wg = sgam[wave]; unsigned int* wc = scnt[wave];
    vg_walk<G>(x, y, v, n, d0, sxy, sv, [&](double dx, double dy, const VgVals<G>& vi, const double* vj) {
        const double h = sqrt(vg_dist2(dx, dy));
        int k = vg_below(se, h);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (per_date && g > 0) k = vg_below(se + g * VG_EPAD, h);
            const double a = vi.v[g], b = vj[g];
            if (k >= 1 && k <= nbins && a == a && b == b) {        // edges[k - 1] < h <= edges[k]
                double gam;
                {
#pragma clang fp contract(off)
                    const double d = a - b;
                    gam = 0.5 * (d * d);
                }
                const int o = g * VG_MAXB + k - 1;
                atomicAdd(&wc[o], 1u);
                __hip_atomic_fetch_add(&wl[o], h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(&wg[o], gam, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    });
    __syncthreads();
    for (int k = tid; k < G * nbins; k += VG_TILE) {
        const int o = (k / nbins) * VG_MAXB + k % nbins;
        unsigned long long cnt = 0ull; double l = 0.0, gm = 0.0;
#pragma unroll
        for (int w = 0; w < VG_WAVES; ++w) { cnt += scnt[w][o]; l += slag[w][o]; gm += sgam[w][o]; }
        const size_t q = (size_t)blockIdx.x * (G * nbins) + k;
        part_count[q] = cnt; part_lag[q] = l; part_gamma[q] = gm;
    }
}

// the partials of `nwg` workgroups, added in workgroup order: out[(d0 + g) * nbins + b]
__global__ void pair_reduce_kernel(const unsigned long long* __restrict__ part_count, const double* __restrict__ part_lag,
                                   const double* __restrict__ part_gamma, int nwg, int gb, long long out0,
                                   long long* __restrict__ count, double* __restrict__ lag_sum, double* __restrict__ gamma_sum) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= gb) return;
    unsigned long long cnt = 0ull; double l = 0.0, gm = 0.0;
    for (int w = 0; w < nwg; ++w) { const size_t q = (size_t)w * gb + k; cnt += part_count[q]; l += part_lag[q]; gm += part_gamma[q]; }
    count[out0 + k] = (long long)cnt; lag_sum[out0 + k] = l; gamma_sum[out0 + k] = gm;
}
