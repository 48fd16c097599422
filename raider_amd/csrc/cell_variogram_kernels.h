// Per-grid-cell variograms of a station series in one pass (cli/statsPlot.py:721-814, _append_variogram without its sampling),
// included by raider_hip.hip after variogram_kernels.h, whose vg_dist2, vg_below, +inf-padded edge rows and per-wave LDS histograms
// are reused.
//
// Stations come sorted by cell: cell c owns x, y, values[d][cell_start[c] .. cell_start[c + 1]).  A workgroup of VG_TILE lanes owns ONE
// (cell, group of G <= 4 dates) and runs, with barriers between them and no host round trip,
//   a. per date: the count of valid stations and - when asked - the plane removal over them;
//   b. (default bins) the largest pair distance valid on the date and the row linspace(0, 0.67 hmax, nbins + 1) made from it;
//   c. the all-pair binning; one workgroup owns the slice, so it writes final values - no partials, no second kernel.
// A cell of tens of stations is the usual case: the lanes stride over the LINEAR index of the cell's upper triangle, so 45 stations
// (990 pairs) keep every lane busy for four steps, where an "i per lane" walk would idle 211 of 256.  The (i, j) of a lane is advanced
// incrementally (j += VG_TILE, carried over the rows), not decoded by a square root per pair.
//
// LDS (G = 4): x, y 8 KiB + values 16 KiB + edge rows 4 KiB + per-wave histograms 20 KiB + 1 KiB of reduction scratch = 49 KiB static;
// three workgroups fit in a compute unit's 160 KiB.  A cell of more than CV_LDS_MAX stations runs the same body on its slice in
// global memory (the LDS template flag), its residuals going through the `resid` array.
//
// Plane removal (phase a).  Over the n valid stations of the date: means mx, my, mv; centred moments Sxx, Sxy, Syy, Sxv, Syv, all f64
// workgroup reductions in a fixed order (lane-strided partials, wave shuffles, the four waves added in order: deterministic);
// a = (Syy Sxv - Sxy Syv) / det, b = (Sxx Syv - Sxy Sxv) / det, det = Sxx Syy - Sxy^2; residual (v - mv) - (a (x - mx) + b (y - my)).
// SINGULARITY CRITERION: the slice gets status 2, and is left to the host's lstsq, unless det > CV_SINGULAR * (Sxx + Syy)^2 - that is,
// unless the smaller eigenvalue of the centred normal matrix is above about 1e-12 of the larger (det = their product, Sxx + Syy their sum):
// the valid stations' scatter is wider than 1e-6 of its length.  Invariant under rotation; it catches fewer than three stations, stations
// at one place or on one line in any direction, rounding noise of the coordinates included - where lstsq gives its minimum-norm answer.
//
// status: 0 done, 1 skipped (fewer than min_valid valid stations), 2 singular plane (nothing binned: the host redoes the slice).  A
// slice with status != 0 has count = lag = gamma = 0, hmax NaN and - when the plane is removed - NaN residuals.
#pragma once

constexpr int CV_LDS_MAX = 512;               // stations of a cell that is staged in LDS
constexpr double CV_SINGULAR = 1e-12;

struct CellVgArgs {
    const double *x, *y, *values; const long long* cell_start; long long n; int nd, deramp, min_valid;
    const double* edges; int nbins;           // edges NULL: default row per (cell, date); else [ncells][nbins + 1]
    long long* nvalid; double* hmax; int* status; long long* count; double *lag, *gamma, *edges_out;
    double* resid;                            // [nd][n]; never NULL when deramp
};

template <int G> struct CvShared {
    double x[CV_LDS_MAX], y[CV_LDS_MAX], v[G * CV_LDS_MAX], e[G * VG_EPAD];
    double lag[VG_WAVES][G * VG_MAXB], gam[VG_WAVES][G * VG_MAXB];
    unsigned int cnt[VG_WAVES][G * VG_MAXB];
    double red[VG_WAVES * 5 * G];
    unsigned long long m[G];
};

// a[k] <- the sum of a[k] over the workgroup, in every lane, in a fixed order
template <int K>
__device__ __forceinline__ void cv_reduce(double (&a)[K], double* red) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double w = a[k];
        for (int o = 32; o > 0; o >>= 1) w += __shfl_xor(w, o, 64);
        a[k] = w;
    }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[(threadIdx.x >> 6) * K + k] = a[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) a[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
    __syncthreads();                                      // (red may be written again)
}

// the workgroup's lanes over the pairs i < j of m points, in the order of the linear index p = tid, tid + VG_TILE, ...
template <typename F>
__device__ __forceinline__ void cv_pairs(int m, F&& f) {
    int i = 0, j = 1 + (int)threadIdx.x;
    for (;;) {
        while (j >= m) {                                  // past the end of row i: row i + 1 starts at j = i + 2
            ++i;
            if (i >= m - 1) return;
            j = j - m + i + 1;
        }
        f(i, j);
        j += VG_TILE;
    }
}

template <int G>
__device__ __forceinline__ void cv_merge_max(const unsigned long long (&mx)[G], unsigned long long* sm) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
        unsigned long long w = mx[g];
        for (int o = 32; o > 0; o >>= 1) { const unsigned long long t = __shfl_xor(w, o, 64); w = t > w ? t : w; }
        if ((threadIdx.x & 63) == 0 && w) atomicMax(&sm[g], w);
    }
    __syncthreads();
}

template <int G, bool LDS>
__device__ __forceinline__ void cv_body(const CellVgArgs& A, int cell, int dd, long long s0, int m, CvShared<G>& S) {
    const int tid = threadIdx.x, wave = tid >> 6, nbins = A.nbins, ne = nbins + 1;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
    const double *X, *Y, *V; size_t vs;                   // value of date g at station k of the cell: V[g * vs + k]
    if (tid < G) S.m[tid] = 0ull;
    if (LDS) {
        for (int k = tid; k < m; k += VG_TILE) {
            S.x[k] = A.x[s0 + k]; S.y[k] = A.y[s0 + k];
#pragma unroll
            for (int g = 0; g < G; ++g) S.v[g * CV_LDS_MAX + k] = A.values[(size_t)(dd + g) * A.n + s0 + k];
        }
        X = S.x; Y = S.y; V = S.v; vs = CV_LDS_MAX;
    } else {
        X = A.x + s0; Y = A.y + s0; V = A.values + (size_t)dd * A.n + s0; vs = (size_t)A.n;
    }
    __syncthreads();

    // ---- a. counts, and the plane removal -----------------------------------------------------------------------------------------
    double cnt[G]; int st[G]; bool use[G];
    if (!A.deramp) {
#pragma unroll
        for (int g = 0; g < G; ++g) cnt[g] = 0.0;
        for (int k = tid; k < m; k += VG_TILE)
#pragma unroll
            for (int g = 0; g < G; ++g) { const double v = V[g * vs + k]; cnt[g] += v == v ? 1.0 : 0.0; }
        cv_reduce<G>(cnt, S.red);
#pragma unroll
        for (int g = 0; g < G; ++g) { st[g] = cnt[g] < (double)A.min_valid ? 1 : 0; use[g] = st[g] == 0; }
    } else {
        double a1[4 * G];
#pragma unroll
        for (int q = 0; q < 4 * G; ++q) a1[q] = 0.0;
        for (int k = tid; k < m; k += VG_TILE) {
            const double xk = X[k], yk = Y[k];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const double v = V[g * vs + k];
                if (v == v) { a1[4 * g] += 1.0; a1[4 * g + 1] += xk; a1[4 * g + 2] += yk; a1[4 * g + 3] += v; }
            }
        }
        cv_reduce<4 * G>(a1, S.red);
        double mx[G], my[G], mv[G], a2[5 * G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            cnt[g] = a1[4 * g];
            const double nn = cnt[g] > 0.0 ? cnt[g] : 1.0;
            mx[g] = a1[4 * g + 1] / nn; my[g] = a1[4 * g + 2] / nn; mv[g] = a1[4 * g + 3] / nn;
        }
#pragma unroll
        for (int q = 0; q < 5 * G; ++q) a2[q] = 0.0;
        for (int k = tid; k < m; k += VG_TILE) {
            const double xk = X[k], yk = Y[k];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const double v = V[g * vs + k];
                if (v == v) {
                    const double dx = xk - mx[g], dy = yk - my[g], dv = v - mv[g];
                    a2[5 * g] += dx * dx; a2[5 * g + 1] += dx * dy; a2[5 * g + 2] += dy * dy; a2[5 * g + 3] += dx * dv; a2[5 * g + 4] += dy * dv;
                }
            }
        }
        cv_reduce<5 * G>(a2, S.red);
        double pa[G], pb[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const double sxx = a2[5 * g], sxy = a2[5 * g + 1], syy = a2[5 * g + 2], sxv = a2[5 * g + 3], syv = a2[5 * g + 4];
            const double det = sxx * syy - sxy * sxy;
            const bool sing = !(det > CV_SINGULAR * ((sxx + syy) * (sxx + syy)));
            st[g] = cnt[g] < (double)A.min_valid ? 1 : sing ? 2 : 0;
            use[g] = st[g] == 0;
            pa[g] = use[g] ? (syy * sxv - sxy * syv) / det : 0.0;
            pb[g] = use[g] ? (sxx * syv - sxy * sxv) / det : 0.0;
        }
        __syncthreads();                                  // every lane has read the values it summed
        for (int k = tid; k < m; k += VG_TILE) {
            const double xk = X[k], yk = Y[k];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const double v = V[g * vs + k];
                const double r = use[g] && v == v ? (v - mv[g]) - (pa[g] * (xk - mx[g]) + pb[g] * (yk - my[g])) : qnan;
                if (LDS) S.v[g * CV_LDS_MAX + k] = r;
                A.resid[(size_t)(dd + g) * A.n + s0 + k] = r;
            }
        }
        if (!LDS) V = A.resid + (size_t)dd * A.n + s0;    // (what this workgroup wrote, read back behind the barrier)
        __syncthreads();
    }

    // ---- b. the largest pair distance of each date, and the default rows made from it ----------------------------------------------
    const bool per_date = A.edges == nullptr;
    if (per_date) {
        unsigned long long mx2[G];
#pragma unroll
        for (int g = 0; g < G; ++g) mx2[g] = 0ull;
        cv_pairs(m, [&](int i, int j) {
            const double d2 = vg_dist2(X[i] - X[j], Y[i] - Y[j]);
            if (!(d2 >= 0.0)) return;
            const unsigned long long w = (unsigned long long)__double_as_longlong(d2) + 1ull;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const double a = V[g * vs + i], b = V[g * vs + j];
                if (use[g] && a == a && b == b && w > mx2[g]) mx2[g] = w;
            }
        });
        cv_merge_max<G>(mx2, S.m);
    }
    for (int k = tid; k < G * VG_EPAD; k += VG_TILE) {
        const int g = k / VG_EPAD, c = k % VG_EPAD;
        double e = inf;
        if (c < ne) {
            if (per_date) {
                // np.linspace(0, 0.67 hmax, nbins + 1), bit for bit: step = stop / nbins, k * step, the last one the stop itself
#pragma clang fp contract(off)
                const unsigned long long w = S.m[g];
                const double hm = w ? sqrt(__longlong_as_double((long long)(w - 1ull))) : qnan;
                const double s = hm * 0.67, step = s / (double)nbins;
                const double shown = c < nbins ? (double)c * step : s;
                if (A.edges_out) A.edges_out[((size_t)cell * A.nd + dd + g) * ne + c] = shown;
                // a row without a pair (NaN) or with all stations in one place (0) can catch nothing: any valid row stands in
                e = s > 0.0 ? shown : (c < nbins ? (double)c * (1.0 / (double)nbins) : 1.0);
            } else {
                e = A.edges[(size_t)cell * ne + c];
                if (A.edges_out) A.edges_out[((size_t)cell * A.nd + dd + g) * ne + c] = e;
            }
        }
        S.e[k] = e;
    }
    for (int k = tid; k < VG_WAVES * G * VG_MAXB; k += VG_TILE) { (&S.lag[0][0])[k] = 0.0; (&S.gam[0][0])[k] = 0.0; (&S.cnt[0][0])[k] = 0u; }
    __syncthreads();

    // ---- c. the bins ---------------------------------------------------------------------------------------------------------------
    double* wl = S.lag[wave]; double* wg = S.gam[wave]; unsigned int* wc = S.cnt[wave];
    unsigned long long mx2[G];
#pragma unroll
    for (int g = 0; g < G; ++g) mx2[g] = 0ull;
    cv_pairs(m, [&](int i, int j) {
        const double d2 = vg_dist2(X[i] - X[j], Y[i] - Y[j]);
        if (!(d2 >= 0.0)) return;
        const double h = sqrt(d2);
        const unsigned long long w = (unsigned long long)__double_as_longlong(d2) + 1ull;
        int k = vg_below(S.e, h);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (per_date && g > 0) k = vg_below(S.e + g * VG_EPAD, h);
            const double a = V[g * vs + i], b = V[g * vs + j];
            if (!(use[g] && a == a && b == b)) continue;
            if (!per_date && w > mx2[g]) mx2[g] = w;      // (given rows: the largest distance comes out of this one pass)
            if (k >= 1 && k <= nbins) {                   // edges[k - 1] < h <= edges[k]
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
    if (!per_date) cv_merge_max<G>(mx2, S.m); else __syncthreads();
    for (int k = tid; k < G * nbins; k += VG_TILE) {
        const int g = k / nbins, o = g * VG_MAXB + k % nbins;
        unsigned long long c = 0ull; double l = 0.0, gm = 0.0;
#pragma unroll
        for (int w = 0; w < VG_WAVES; ++w) { c += S.cnt[w][o]; l += S.lag[w][o]; gm += S.gam[w][o]; }
        const size_t q = ((size_t)cell * A.nd + dd + g) * nbins + k % nbins;
        A.count[q] = (long long)c; A.lag[q] = l; A.gamma[q] = gm;
    }
    if (tid < G) {
        // (use[], st[], cnt[] are the same in every lane; indexed by a constant below to stay in registers)
        const size_t q = (size_t)cell * A.nd + dd + tid;
        const unsigned long long w = S.m[tid];
        A.hmax[q] = w ? sqrt(__longlong_as_double((long long)(w - 1ull))) : qnan;
#pragma unroll
        for (int g = 0; g < G; ++g)
            if (g == tid) { A.nvalid[q] = (long long)cnt[g]; A.status[q] = st[g]; }
    }
}

// workgroup b: cell b / ngroups, dates d0 + (b % ngroups) * G .. + G
template <int G>
__global__ __launch_bounds__(VG_TILE) void cell_variogram_kernel(CellVgArgs A, int d0, int ngroups) {
    __shared__ CvShared<G> S;
    const int cell = blockIdx.x / ngroups, dd = d0 + (blockIdx.x % ngroups) * G;
    const long long s0 = A.cell_start[cell];
    const int m = (int)(A.cell_start[cell + 1] - s0);
    if (m <= CV_LDS_MAX) cv_body<G, true>(A, cell, dd, s0, m, S);
    else cv_body<G, false>(A, cell, dd, s0, m, S);
}

// tot[c][b] = the slices of cell c with status 0, added in date order
__global__ void cell_totals_kernel(const long long* __restrict__ count, const double* __restrict__ lag, const double* __restrict__ gamma,
                                   const int* __restrict__ status, int ncells, int nd, int nbins, long long* __restrict__ tot_count,
                                   double* __restrict__ tot_lag, double* __restrict__ tot_gamma) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (long long)ncells * nbins) return;
    const int c = (int)(k / nbins), b = (int)(k % nbins);
    long long n = 0; double l = 0.0, g = 0.0;
    for (int d = 0; d < nd; ++d) {
        if (status[(size_t)c * nd + d] != 0) continue;
        const size_t q = ((size_t)c * nd + d) * nbins + b;
        n += count[q]; l += lag[q]; g += gamma[q];
    }
    tot_count[k] = n; tot_lag[k] = l; tot_gamma[k] = g;
}
