// Device-side building blocks of libraider_hip (gfx950 / CDNA4 only).
//
//   CubeView + locate /        scipy RegularGridInterpolator(linear, fill=nan) on the interleaved (wet,hydro) cube
//   corner_weights / _sum      [delayFcns.py:55-56, scipy _rgi.py:405-499]: the pieces every point gather shares (cube_kernels.h)
//   sample_issue / _finish     the same interpolation for the ray kernels, split so that several samples' gathers fly together
//   toa_newton / _t            getTopOfAtmosphere [losreader.py:706-733] (materialising API kernels / generic ray kernels)
//   crossings_kernel           pass 1: build_ray [losreader.py:772-835] -> per-level batch maximum of the ray length
//                              (delay.py:283) + NaN / z-clamp flags (delay.py:279,306-311) + the ray records for pass 2
//   march_slice_levels /       pass 2: the two level loops of the light rays over E cubes on one ray geometry, called by
//   march_ray_height_levels    march_kernel (E = 1) and by march_epochs_kernel (epoch_kernels.h, E epochs of a date series)
//   march_kernel               pass 2: the trapezoid of _build_cube_ray [delay.py:285-323]
//   trace_kernel               both in one kernel, for one slice of GRID rays with look vectors on an f32 lon/lat cube with exactly
//                              uniform axes: pass 1's tile body (pass1_tiles, written once for both kernels) folds the exact maxima and
//                              marches the tile from registers on a PROBED partition (crossings_kernel over RayParams::tile_list,
//                              level_table_kernel, partition_check_kernel<false>); partition_check_kernel<true> then proves the partition
//                              from the exact maxima or sends the call through the two passes enqueued behind (RayParams::one_pass)
//
// Design notes (MI355X):
//   * one ray per lane, 64-lane wavefronts, 256-thread workgroups = one 16x16 pixel tile of the scene: neighbouring rays
//     walk the same few cube columns, so their gathers hit the same L1/L2 lines; everything that depends only on the slice
//     (levels, nParts, the sample schedule) is wave-uniform and lives in SGPRs / LDS, so a wave never diverges.
//   * light rays (almost all): height, latitude and longitude along the ray are degree-5 polynomials of the ray parameter
//     fitted once per ray from six full geodesy evaluations (geodesy_fast.h); level crossings and samples are then FMAs.
//     The few rays the static classification rejects (poles, grazing incidence, +-180 deg) take the generic kernels.
//   * the cube is stored (y,x,z) with z fastest and (wet,hydro) interleaved per cell: the two z neighbours of both fields
//     of one column are ONE contiguous 16 B (f32) / 32 B (f64) read, four per sample against uniform row bases.
//   * grid axes + the level table + the per-level partition live in LDS (a few KB), filled once per workgroup; nothing
//     per-level is ever materialised in HBM (the reference materialises K x N x 56 B).
//   * persistent grid (a few workgroups per CU) walking tiles with an XCD-aware mapping so that the 32 CUs sharing one L2
//     work on one contiguous band of the scene.
//   * no MFMA: this is a gather + fp64 polynomial/interpolation integrate, there is no contraction.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "geodesy.h"
#include "geodesy_fast.h"

namespace rdr {

constexpr int TILE = 16;         // 16x16 pixel tile per workgroup (GRID mode)
constexpr int BLOCK = TILE * TILE;
constexpr int MAX_LEVELS = 512;  // model intervals (ERA5 has 144)
constexpr int MAX_NPARTS = 65536; // integration points per model interval (guards the sample loop against diverged ray lengths)

template <typename T2>
struct CubeView {
    const T2* v;          // [(iy*nx+ix)*nz+iz] -> (wet, hydro)
    const double* axes;   // ys[ny] | xs[nx] | zs[nz]   (ascending)
    int ny, nx, nz;
    double y_lo, y_hi, x_lo, x_hi, z_lo, z_hi;   // axis end points (bounds test)
    double inv_dy, inv_dx, inv_dz;               // (n-1)/(g[n-1]-g[0]) for the uniform-axis index guess
    int uni_y, uni_x, uni_z;                     // axis is (nearly) uniform: guess is within +-1 cell
    int exact_y, exact_x;                        // axis is uniform to round-off: the cell follows from arithmetic alone
    int small;                                   // ny*nx < 2^24, nz < 2^24 and the field fits 4 GB: 32-bit index arithmetic
};

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }

// index i with g[i] <= x < g[i+1], clamped to [0, n-2] (last cell closed) - scipy find_indices.
__device__ __forceinline__ int find_cell(const double* g, int n, double x, double g0, double inv_d, int uniform) {
    int i;
    if (uniform) {
        i = (int)((x - g0) * inv_d);
        i = min(max(i, 0), n - 2);
        while (i > 0 && x < g[i]) --i;
        while (i < n - 2 && x >= g[i + 1]) ++i;
    } else {
        int lo = 0, hi = n;   // first index with x < g[idx]
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (x < g[mid]) hi = mid; else lo = mid + 1;
        }
        i = min(max(lo - 1, 0), n - 2);
    }
    return i;
}

__device__ __forceinline__ void ld2(const float2* p, double& a, double& b) { const float2 t = *p; a = (double)t.x; b = (double)t.y; }
__device__ __forceinline__ void ld2(const double2* p, double& a, double& b) { const double2 t = *p; a = t.x; b = t.y; }

// ---- the point gather's shared pieces (zenith / station kernels) ---------------------------------------------------------------------
// scipy linear RGI on both fields, written once: every point-gather kernel (gather_points of cube_kernels.h: the plain, paired, blended,
// quad and date-series routes) is gather_axes + locate + corner_weights + corner_sum around its own corner loads, so the routes give the
// same bits because they run the same code.

// The three axes: copied into LDS when they fit (axes_in_lds), else read from global memory (L1 / L2 hits).
struct GatherAxes { const double *y, *x, *z; };

template <typename T2>
__device__ __forceinline__ GatherAxes gather_axes(const CubeView<T2>& c, unsigned char* smem_raw, int axes_in_lds) {
    const double* s_y = c.axes;
    if (axes_in_lds) {
        double* t = reinterpret_cast<double*>(smem_raw);
        for (int i = threadIdx.x; i < c.ny + c.nx + c.nz; i += blockDim.x) t[i] = c.axes[i];
        __syncthreads();
        s_y = t;
    }
    return {s_y, s_y + c.ny, s_y + c.ny + c.nx};
}

// A located point: its cell (the lower corner's node indices) and the fractions along the three axes.
struct GatherCell { int iy, ix, iz; double ty, tx, tz; };

// false: out of bounds (x < g[0] or x > g[-1]) -> fill_value nan; nan coordinate -> nan   (_rgi.py:437-442,585-592)
template <typename T2>
__device__ __forceinline__ bool locate(const CubeView<T2>& c, const GatherAxes& s, double y, double x, double z, GatherCell& L) {
    const bool inside = (y >= c.y_lo) && (y <= c.y_hi) && (x >= c.x_lo) && (x <= c.x_hi) && (z >= c.z_lo) && (z <= c.z_hi);
    if (!inside) return false;
    L.iy = find_cell(s.y, c.ny, y, c.y_lo, c.inv_dy, c.uni_y);
    L.ix = find_cell(s.x, c.nx, x, c.x_lo, c.inv_dx, c.uni_x);
    L.iz = find_cell(s.z, c.nz, z, c.z_lo, c.inv_dz, c.uni_z);
    L.ty = (y - s.y[L.iy]) / (s.y[L.iy + 1] - s.y[L.iy]);
    L.tx = (x - s.x[L.ix]) / (s.x[L.ix + 1] - s.x[L.ix]);
    L.tz = (z - s.z[L.iz]) / (s.z[L.iz + 1] - s.z[L.iz]);
    return true;
}

// weight = ((1*wy)*wx)*wz, corners in lexicographic (y,x,z) order   (_rgi.py:490-498)
__device__ __forceinline__ void corner_weights(double ty, double tx, double tz, double (&k)[8]) {
    const double wy0 = 1.0 - ty, wx0 = 1.0 - tx, wz0 = 1.0 - tz;
    const double a00 = wy0 * wx0, a01 = wy0 * tx, a10 = ty * wx0, a11 = ty * tx;
    k[0] = a00 * wz0; k[1] = a00 * tz; k[2] = a01 * wz0; k[3] = a01 * tz;
    k[4] = a10 * wz0; k[5] = a10 * tz; k[6] = a11 * wz0; k[7] = a11 * tz;
}

// value = 0 + sum over the corners in that order (_rgi.py:490-498): per field one v_fma_f64 on 0 and seven v_fmac_f64
__device__ __forceinline__ void corner_sum(const double (&w)[8], const double (&h)[8], const double (&k)[8], double& wet, double& hyd) {
    double sw = 0.0, sh = 0.0;
    sw += w[0] * k[0]; sh += h[0] * k[0];
    sw += w[1] * k[1]; sh += h[1] * k[1];
    sw += w[2] * k[2]; sh += h[2] * k[2];
    sw += w[3] * k[3]; sh += h[3] * k[3];
    sw += w[4] * k[4]; sh += h[4] * k[4];
    sw += w[5] * k[5]; sh += h[5] * k[5];
    sw += w[6] * k[6]; sh += h[6] * k[6];
    sw += w[7] * k[7]; sh += h[7] * k[7];
    wet = sw; hyd = sh;
}

// LDS-resident axis tables of the ray kernels: (g[i], 1/(g[i+1]-g[i])) pairs per axis; ey / ex are null for exact axes
struct AxisTabs { const double2* ey; const double2* ex; const double2* ez; };

// ---- ray-kernel sampler ----------------------------------------------------------------------------------------
// Same scipy semantics as locate (interval g[i] <= v < g[i+1], last cell closed; outside / NaN -> NaN).
// The axis table is stored in LDS as (g[i], 1/(g[i+1]-g[i])) pairs.  x / y: arithmetic cell on exactly-uniform axes,
// guess-and-verify on nearly uniform ones; z: the segment's model interval is known, a 2- (light kernel) or 3-entry
// (generic kernel) window around it is fetched and the right entry selected in registers.  A lane whose guess fails
// (irregular axis, non-converged crossing in sub-metre levels, < 4-node axes, outside the grid) searches exactly.
__device__ __forceinline__ int bisect_cell2(const double2* e, int n, double v) {
    int lo = 0, hi = n;   // first index with v < g[idx]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v < e[mid].x) hi = mid; else lo = mid + 1;
    }
    return min(max(lo - 1, 0), n - 2);
}

// Exact cell search (scipy find_indices semantics) - the rare path of the two fast searches below.  A coordinate outside
// the axis (or NaN) gets a NaN weight, which makes the interpolated values NaN = scipy's fill_value (_rgi.py:437-442,585-592).
__device__ __forceinline__ void cell_exact(const double2* e, int n, double v, int& i, double& t) {
    if (!((v >= e[0].x) & (v <= e[n - 1].x))) { i = 0; t = qnan(); return; }
    i = bisect_cell2(e, n, v);
    t = (v - e[i].x) * e[i].y;
}

__device__ __forceinline__ void window_cell(const double2* e, int n, double v, int guess, bool trust, int& i, double& t) {
    const int i0 = min(max(guess, 1), n - 3);
    const double2 em = e[i0 - 1], e0 = e[i0], e1 = e[i0 + 1];
    const bool dn = v < e0.x, up = v >= e1.x;
    i = i0 - (int)dn + (int)up;
    const double g = dn ? em.x : (up ? e1.x : e0.x);
    const double r = dn ? em.y : (up ? e1.y : e0.y);
    t = (v - g) * r;
    if (!trust || !(t >= 0.0) || !(t <= 1.0)) cell_exact(e, n, v, i, t);      // rare
}

// The sample is known to sit in model interval `guess` or - within the Newton residual of a level crossing - just above its
// top node (every evaluated sample but a ray's very first one is interior to its segment or its TOP end): two table
// entries decide.  Anything else (t outside [0,1]) falls back to the exact search.
__device__ __forceinline__ int window2_base(int n, int guess) { return min(max(guess, 0), n - 3); }

__device__ __forceinline__ void window2_cell(const double2* e, int n, double v, int i0, bool trust, int& i, double& t) {
    const double2 e0 = e[i0], e1 = e[i0 + 1];                                 // i0 = window2_base(n, guess), slice-uniform
    // measured from the MIDDLE node g[i0+1] (where a level top sits, within the Newton residual): above it the weight is d r1,
    // below it 1 + d r0 - one subtraction, one 64-bit select (the reciprocal), one 32-bit select (the high word of 0.0 / 1.0)
    const double d = v - e1.x;
    const bool up = d >= 0.0;
    i = i0 + (int)up;
    t = fma(d, up ? e1.y : e0.y, up ? 0.0 : 1.0);
    if (!trust || !(t >= 0.0) || !(t <= 1.0)) cell_exact(e, n, v, i, t);      // rare
}

// x / y axes.  `exact` (axis uniform to round-off, the usual lat/lon grid): the cell index and the weight come from
// (v - g0) * (n-1)/(g[n-1]-g0) alone - no table access; they differ from scipy's (v - g[i])/(g[i+1]-g[i]) by the axis's own
// round-off (<= 1e-11 of a cell, checked on the host), which the continuous interpolant turns into <= 1e-12 relative.
// Otherwise (nearly uniform axis): read the guessed cell and the next node from the LDS table and verify.
// Anything else (last node, outside, NaN, irregular axis) takes the exact search.
// IDX (light rays on an exact axis): v already IS the index-space coordinate (v_real - g0) * inv_d - pass 1 folds that map
// into the ray polynomial's coefficients.
// NOCHECK (light march loop, exact axes only): the caller has PROVEN from the ray's polynomial coefficients that every sample of
// every ray of the wave lies inside [0, n-1) - the bounds test and its rare path are compiled out.
template <bool IDX = false, bool NOCHECK = false>
__device__ __forceinline__ void cell_xy(const double2* e, int n, double v, double g0, double g_last, double inv_d, bool exact, bool trust,
                                        int& i, double& t) {
    bool ok;
    const double tf = (IDX && exact) ? v : (v - g0) * inv_d;
    if (exact) {
        i = (int)tf;                                                            // = floor for the tf >= 0 this path accepts
        t = __builtin_amdgcn_fract(tf);
        if (NOCHECK) return;
        const double nm1 = (double)(n - 1);
        ok = (tf >= 0.0) & (tf < nm1);
        if (__builtin_expect(!ok, 0)) {                                         // rare: the last node, outside the axis, NaN
            asm volatile("" ::: "memory");                                      // keep this a skipped branch, not if-converted selects
            // inside the axis after all?  In axis units when v is one (scipy's own test, _rgi.py:437-442); an index-space
            // coordinate (IDX) is inside only ON the last node.  The cell follows from which end tf fell off: a coordinate a
            // rounding error below the first node belongs to cell 0, not to the last cell.
            const bool inside = IDX ? (tf == nm1) : ((v >= g0) & (v <= g_last));
            const bool low_end = tf < 1.0;
            i = (inside && !low_end) ? n - 2 : 0;
            t = inside ? (low_end ? tf : (tf - nm1) + 1.0) : qnan();
        }
        return;
    } else {
        // one table entry: the weight itself says whether the guess was the cell (t in [0, 1)); anything else - the neighbour
        // cell, the last node, outside, NaN - takes the exact search.  (A v exactly ON node i+1 may be accepted here with
        // t = 1 - 1 ulp instead of cell i+1 with t = 0: the same value of the continuous interpolant.)
        i = min(max((int)tf, 0), n - 2);
        const double2 e0 = e[i];
        t = (v - e0.x) * e0.y;
        ok = trust & (t >= 0.0) & (t < 1.0);
    }
    if (!ok) cell_exact(e, n, v, i, t);                                         // rare
}

// One trilinear sample in two halves, so that several samples' gathers can be in flight together:
//   sample_issue : cell search on the three axes, address, the four 16-byte (32-byte for f64 cubes) corner-pair loads
//   sample_finish: weights, f32->f64 conversion, the 16 FMAs                    (weights/corner order: _rgi.py:490-498)
// E samples that share their cell and weights - one set of corners per weather epoch of a series (epoch_kernels.h); E = 1: one cube.
template <typename T2, int E = 1>
struct PendingSample {
    T2 v[E][8];           // per epoch: corners in (y,x,z) lexicographic order
    double ty, tx, tz;
};

// The value pointers of E cubes of one shape (a kernel argument of the stacked kernels); E = 1: the cube's own c.v.
template <typename T2, int E>
struct EpochCubes { const T2* v[E]; };

// The horizontal half of a sample: cell search on x / y (cell_xy) and the element offset of corner (iy, ix, iz), both once, then per
// cube the four 16-byte (32-byte for f64 cubes) corner-pair loads - E x 4 independent loads.  iz may be slice-uniform (a scalar) or
// per lane.
template <typename T2, int E, bool IDX, bool NOCHECK>
__device__ __forceinline__ void gather_corners(const CubeView<T2>& c, const EpochCubes<T2, E>& ev, const AxisTabs& m, double y, double x, int iz,
                                               PendingSample<T2, E>& s) {
    int iy, ix;
    cell_xy<IDX, NOCHECK>(m.ey, c.ny, y, c.y_lo, c.y_hi, c.inv_dy, c.exact_y, c.uni_y, iy, s.ty);
    cell_xy<IDX, NOCHECK>(m.ex, c.nx, x, c.x_lo, c.x_hi, c.inv_dx, c.exact_x, c.uni_x, ix, s.tx);
    if (c.small) {              // one 32-bit element offset against four uniform row bases
        // (iy nx + ix) as ONE full-rate v_mad_u32_u24: left to itself the compiler picks v_mad_u64_u32, a quarter-rate instruction
        // that holds the vector ALU for four issue slots
        unsigned col;
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(col) : "v"((unsigned)iy), "s"((unsigned)c.nx), "v"((unsigned)ix));
        const unsigned off = (__umul24(col, (unsigned)c.nz) + (unsigned)iz) * (unsigned)sizeof(T2);
        const size_t rowx = (size_t)c.nz * sizeof(T2), rowy = (size_t)c.nx * rowx;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const char* b = reinterpret_cast<const char*>(ev.v[e]);
            const T2* p00 = reinterpret_cast<const T2*>(b + off);
            const T2* p01 = reinterpret_cast<const T2*>(b + rowx + off);
            const T2* p10 = reinterpret_cast<const T2*>(b + rowy + off);
            const T2* p11 = reinterpret_cast<const T2*>(b + rowy + rowx + off);
            s.v[e][0] = p00[0]; s.v[e][1] = p00[1];
            s.v[e][2] = p01[0]; s.v[e][3] = p01[1];
            s.v[e][4] = p10[0]; s.v[e][5] = p10[1];
            s.v[e][6] = p11[0]; s.v[e][7] = p11[1];
        }
    } else {
        const int64_t o00 = ((int64_t)iy * c.nx + ix) * c.nz + iz, o01 = o00 + c.nz;
        const int64_t o10 = o00 + (int64_t)c.nx * c.nz, o11 = o10 + c.nz;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const T2* p = ev.v[e];
            s.v[e][0] = p[o00]; s.v[e][1] = p[o00 + 1];
            s.v[e][2] = p[o01]; s.v[e][3] = p[o01 + 1];
            s.v[e][4] = p[o10]; s.v[e][5] = p[o10 + 1];
            s.v[e][6] = p[o11]; s.v[e][7] = p[o11 + 1];
        }
    }
}

// MODE 0: generic kernels (three-entry z window).  MODE 1 (light march loop, a level's TOP sample or the ray's first sample):
// index-space x / y on exact axes, two-entry z window.  MODE 2 (light march loop, a sample strictly INSIDE model interval kz):
// its z cell is kz itself, one table entry, no select.  Any sample whose weight leaves [0,1] takes the exact search.
template <typename T2, int MODE = 0, bool NOCHECK = false, int E = 1>
__device__ __forceinline__ void sample_issue(const CubeView<T2>& c, const EpochCubes<T2, E>& ev, const AxisTabs& m, double y, double x, double z, int kz,
                                             PendingSample<T2, E>& s) {
    const double2* ez = m.ez;
    int iz;
    if (MODE == 2) {
        const double2 e0 = ez[kz];                                              // kz <= nz-2: slice-uniform address
        iz = kz;
        s.tz = (z - e0.x) * e0.y;
        if (!(s.tz >= 0.0) || !(s.tz <= 1.0)) cell_exact(ez, c.nz, z, iz, s.tz);   // rare
    } else if (MODE == 1) window2_cell(ez, c.nz, z, kz, c.nz >= 4, iz, s.tz);
    else window_cell(ez, c.nz, z, kz, c.nz >= 4, iz, s.tz);
    gather_corners<T2, E, MODE != 0, NOCHECK>(c, ev, m, y, x, iz, s);
}

// one cube: its own values
template <typename T2, int MODE = 0, bool NOCHECK = false>
__device__ __forceinline__ void sample_issue(const CubeView<T2>& c, const AxisTabs& m, double y, double x, double z, int kz, PendingSample<T2>& s) {
    sample_issue<T2, MODE, NOCHECK, 1>(c, EpochCubes<T2, 1>{{c.v}}, m, y, x, z, kz, s);
}

// Generic kernels: scipy's own summation order, weight = ((1*wy)*wx)*wz over the corners in lexicographic order (_rgi.py:490-498).
// (e: the epoch of the sample set, here and in sample_finish_lerp)
template <typename T2, int E>
__device__ __forceinline__ void sample_finish(const PendingSample<T2, E>& s, double& wet, double& hyd, int e = 0) {
    const T2* v = s.v[e];
    const double wy0 = 1.0 - s.ty, wx0 = 1.0 - s.tx, wz0 = 1.0 - s.tz;
    const double a00 = wy0 * wx0, a01 = wy0 * s.tx, a10 = s.ty * wx0, a11 = s.ty * s.tx;
    double sw = 0.0, sh = 0.0, k;
    k = a00 * wz0;  sw = fma((double)v[0].x, k, sw); sh = fma((double)v[0].y, k, sh);
    k = a00 * s.tz; sw = fma((double)v[1].x, k, sw); sh = fma((double)v[1].y, k, sh);
    k = a01 * wz0;  sw = fma((double)v[2].x, k, sw); sh = fma((double)v[2].y, k, sh);
    k = a01 * s.tz; sw = fma((double)v[3].x, k, sw); sh = fma((double)v[3].y, k, sh);
    k = a10 * wz0;  sw = fma((double)v[4].x, k, sw); sh = fma((double)v[4].y, k, sh);
    k = a10 * s.tz; sw = fma((double)v[5].x, k, sw); sh = fma((double)v[5].y, k, sh);
    k = a11 * wz0;  sw = fma((double)v[6].x, k, sw); sh = fma((double)v[6].y, k, sh);
    k = a11 * s.tz; sw = fma((double)v[7].x, k, sw); sh = fma((double)v[7].y, k, sh);
    wet = sw; hyd = sh;
}

// Light march loop: the same trilinear interpolant in nested-lerp form, a + t (b - a) along z, then x, then y: 7 lerps of
// (sub, fma) per field = 28 instructions instead of the 31 of the weight-product form (the f32 -> f64 conversions are exact, so
// the two forms agree to a few ulp of the interpolated value; the parity tests hold 1e-9 m on the integrated delay).
template <typename T2, int E>
__device__ __forceinline__ void sample_finish_lerp(const PendingSample<T2, E>& s, double& wet, double& hyd, int e = 0) {
    const T2* v = s.v[e];
    auto lerp = [](double a, double b, double t) { return fma(t, b - a, a); };
    const double w00 = lerp((double)v[0].x, (double)v[1].x, s.tz), h00 = lerp((double)v[0].y, (double)v[1].y, s.tz);
    const double w01 = lerp((double)v[2].x, (double)v[3].x, s.tz), h01 = lerp((double)v[2].y, (double)v[3].y, s.tz);
    const double w10 = lerp((double)v[4].x, (double)v[5].x, s.tz), h10 = lerp((double)v[4].y, (double)v[5].y, s.tz);
    const double w11 = lerp((double)v[6].x, (double)v[7].x, s.tz), h11 = lerp((double)v[6].y, (double)v[7].y, s.tz);
    const double w0 = lerp(w00, w01, s.tx), h0 = lerp(h00, h01, s.tx);
    const double w1 = lerp(w10, w11, s.tx), h1 = lerp(h10, h11, s.tx);
    wet = lerp(w0, w1, s.ty); hyd = lerp(h0, h1, s.ty);
}

template <typename T2>
__device__ __forceinline__ void sample_cube(const CubeView<T2>& c, const AxisTabs& m, double y, double x, double z, int kz,
                                            double& wet, double& hyd) {
    PendingSample<T2> s;
    sample_issue(c, m, y, x, z, kz, s);
    sample_finish(s, wet, hyd);
}

// getTopOfAtmosphere (losreader.py:706-733): pos = xyz + h*los; repeat: pos += los*((h - height(pos))/factor).
// Straight restatement with the PROJ-formula height (used by the materialising API kernels rdr_top_of_atmosphere /
// rdr_build_ray, whose OUTPUT is positions: they match the reference's to ~1e-8 m).
__device__ __forceinline__ void toa_newton(double ox, double oy, double oz, double lx, double ly, double lz,
                                           double h, int iters, double factor, double& px, double& py, double& pz) {
    px = ox + h * lx; py = oy + h * ly; pz = oz + h * lz;
    for (int it = 0; it < iters; ++it) {
        const double hgt = ecef_height(px, py, pz);
        const double step = (h - hgt) / factor;
        px = px + lx * step; py = py + ly * step; pz = pz + lz * step;
    }
}

// Generic ray kernels: the same iteration carried on the scalar ray parameter t (pos = o + t*l): t0 = h,
// t += (h - height(o + t l)) / factor - identical in exact arithmetic to losreader.py:724-731, 2 live doubles per crossing
// instead of 6 - with the PROJ-formula height.
__device__ __forceinline__ double toa_newton_t(double ox, double oy, double oz, double lx, double ly, double lz,
                                               double h, int iters, double inv_factor) {
    double t = h;
#pragma unroll 1
    for (int it = 0; it < iters; ++it) {
        const double hgt = ecef_height(fma(t, lx, ox), fma(t, ly, oy), fma(t, lz, oz));
        t = fma(h - hgt, inv_factor, t);
    }
    return t;
}

// Top crossing of a model level on a light ray: getTopOfAtmosphere's 3 iterations (losreader.py:724-731,817-819) on the
// normalised ray parameter u, with the height from the ray's polynomial.  gain = su / cos_factor.  Used by BOTH passes
// (same instruction sequence -> identical crossings).
__device__ __forceinline__ double level_top_u(const double* hpoly, double hi, double su, double ou, double gain) {
    double u = fma(hi, su, ou);
#pragma unroll
    for (int it = 0; it < 3; ++it) u = fma(hi - poly5(hpoly, u), gain, u);
    return u;
}

// N independent level crossings carried side by side (same arithmetic per level as level_top_u).
template <int N>
__device__ __forceinline__ void level_top_u_n(const double* hpoly, const double* hi, double su, double ou, double gain, double* u) {
#pragma unroll
    for (int j = 0; j < N; ++j) u[j] = fma(hi[j], su, ou);
#pragma unroll
    for (int it = 0; it < 3; ++it) {
        double p[N];
#pragma unroll
        for (int j = 0; j < N; ++j) p[j] = hpoly[PN - 1];
#pragma unroll
        for (int n = PN - 2; n >= 0; --n) {
#pragma unroll
            for (int j = 0; j < N; ++j) p[j] = fma(p[j], u[j], hpoly[n]);
        }
#pragma unroll
        for (int j = 0; j < N; ++j) u[j] = fma(hi[j] - p[j], gain, u[j]);
    }
}

// ---- crossing polynomial ---------------------------------------------------------------------------------------------
// The (deliberately NOT converged) three-iteration crossing level_top_u(h) of a light ray is a composition of polynomials in
// the level height h, i.e. a smooth function of h; its degree-7 interpolant X(v) at the 8 Chebyshev nodes of the slice's
// level-top range, v = (h - hm) / hh in [-1, 1], reproduces it to < 1e-10 m along the ray up to 60 deg incidence, 7e-9 m at
// 70 deg and 3e-6 m at 85 deg under an 80 km model top (a crossing shifted by d moves a delay by ~1.5e-3 d; sweep:
// tools/ray_poly_probe.py).  Pass 1 fits it once per ray (8 x 21 FMAs + 64) and then every level crossing, in BOTH passes,
// is 7 FMAs instead of 21 - same polynomial, same level abscissae (LDS table xv), hence identical crossings in the two passes.
constexpr int PX = 8;
__device__ const double XPOLY_NODES[PX] = {0.98078528040323044913, 0.83146961230254523708, 0.55557023301960222474, 0.19509032201612826785,
                                           -0.19509032201612826785, -0.55557023301960222474, -0.83146961230254523708, -0.98078528040323044913};
__device__ const double XPOLY_VINV[PX][PX] = {   // [node j][power n]
    {-0.024864045922457250864, -0.025351161379823003334, 0.76980164952545230204, 0.78488295543032986324, -3.1779876260079822119, -3.2402480843731826008, 3.0614674589207181738, 3.1214451522580522856},
    {0.083522329739912365, 0.10045145186799834205, -2.5519026177451504679, -3.0691471822744071686, 9.6723408277623460247, 11.632825402935940496, -7.391036260090294049, -8.8891237283136355959},
    {-0.1870757203331861272, -0.33672740045197043705, 5.3803297424913405655, 9.6843376817517615307, -12.500767952508536122, -22.500787856406753567, 7.391036260090294049, 13.303513796840723793},
    {0.62841743651573101306, 3.2211615113525685678, -3.5982287742716423996, -18.443912220177554698, 6.0064147507541723095, 30.787866300500633524, -3.0614674589207181738, -15.692564486451687186},
    {0.62841743651573101306, -3.2211615113525685678, -3.5982287742716423996, 18.443912220177554698, 6.0064147507541723095, -30.787866300500633524, -3.0614674589207181738, 15.692564486451687186},
    {-0.1870757203331861272, 0.33672740045197043705, 5.3803297424913405655, -9.6843376817517615307, -12.500767952508536122, 22.500787856406753567, 7.391036260090294049, -13.303513796840723793},
    {0.083522329739912365, -0.10045145186799834205, -2.5519026177451504679, 3.0691471822744071686, 9.6723408277623460247, -11.632825402935940496, -7.391036260090294049, 8.8891237283136355959},
    {-0.024864045922457250864, 0.025351161379823003334, 0.76980164952545230204, -0.78488295543032986324, -3.1779876260079822119, 3.2402480843731826008, 3.0614674589207181738, -3.1214451522580522856}};

__device__ __forceinline__ double poly7(const double* c, double v) {
    double r = fma(c[7], v, c[6]);
    r = fma(r, v, c[5]);
    r = fma(r, v, c[4]);
    r = fma(r, v, c[3]);
    r = fma(r, v, c[2]);
    r = fma(r, v, c[1]);
    return fma(r, v, c[0]);
}

// hm / hh: centre and half width of the slice's level-top range (slice-uniform, fill_tables).  Two nodes per trip: their
// Newton chains are independent and fill each other's dependent-issue bubbles.
__device__ __forceinline__ void fit_crossing_poly(const double* hpoly, double su, double ou, double gain, double hm, double hh, double* xc) {
#pragma unroll
    for (int n = 0; n < PX; ++n) xc[n] = 0.0;
#pragma unroll 1
    for (int j = 0; j < PX; j += 2) {
        double hn[2], un[2];
        hn[0] = fma(hh, XPOLY_NODES[j], hm); hn[1] = fma(hh, XPOLY_NODES[j + 1], hm);
        level_top_u_n<2>(hpoly, hn, su, ou, gain, un);
#pragma unroll
        for (int n = 0; n < PX; ++n) xc[n] = fma(XPOLY_VINV[j + 1][n], un[1], fma(XPOLY_VINV[j][n], un[0], xc[n]));
    }
}

// Workspace record handed from pass 1 (crossings_kernel) to pass 2 (march_kernel): one column per ray SLOT
// (slot = local tile * 256 + thread), field-major so every field access is a perfectly coalesced 512 B per wave:
//   ws[f * nslots + slot],  WS_NFIELDS = 29 fields = 232 B per ray - for every ray, light or generic
//   light ray:   0..5 h(u) | 6..11 lat(u) | 12..17 lon(u) monomial coefficients (index space on exact axes) | 18..25 crossing
//                polynomial X(v) | 26 |l|/su (metres per unit of u; > 0) | 27, 28 u at the bottom / top of the first level
//   generic ray: 0..2 origin ECEF | 3..5 look vector | 6 lat0 | 7 lon0 | 8..11 sin/cos lat0, sin/cos lon0 | 12 index of the ray's
//                column in the SIDE buffer, -1: none | 26 = 0.0, which is what marks the ray as generic
// Side buffer (generic rays only, usually empty): side[k * side_cap + idx] = ray parameter t of level crossing k = 0..K.  A
// generic ray that finds the side buffer full (idx -1) has its crossings recomputed by pass 2 - slower, never wrong.
constexpr int WS_POLY_H = 0, WS_POLY_LAT = 6, WS_POLY_LON = 12, WS_XPOLY = 18, WS_SCALE = 26, WS_U0 = 27, WS_U1 = 28, WS_NFIELDS = 29;
constexpr int WS_ORIGIN = 0, WS_LOS = 3, WS_LAT0 = 6, WS_LON0 = 7, WS_S0 = 8, WS_C0 = 9, WS_SL0 = 10, WS_CL0 = 11, WS_SIDE = 12;

struct LevelRec;
struct RayParams {
    // geometry
    int64_t n;
    int origin_mode, los_mode;
    int64_t nx, ny;
    const double* xpts; const double* ypts;
    const double* lat; const double* lon; const double* xyz;
    const double* los; const double* inc; const double* hd;
    double inc0, hd0;
    // slices: a batch is nslices >= 1 height slices of the SAME origins (delay.py:256: one slice per output height).  Tiles are
    // numbered slice-major (tile t belongs to slice t / tiles_per_slice); everything the reference reduces over a slice -
    // per-level maxima, flags, nParts - is kept per slice, so a batched launch gives exactly what slice-by-slice launches give.
    int nslices; int64_t tiles_per_slice;
    const double* hts;                 // [nslices] slice heights, or nullptr: one slice at `ht`
    const double* ht_ray;              // [n] per-ray origin heights (one slice only), or nullptr.  The slice's level table is then built
                                       // for `ht` <= min(ht_ray); ray i joins it at its own first contributing level (first_level)
    int64_t los_stride;                // rays between consecutive slices in los / inc / hd (0: the same arrays for every slice)
    double ht, zref, max_seg;
    // batch-global state
    unsigned long long* maxlen_bits;   // [nslices][MAX_LEVELS] per-level max ray length (bit pattern of a non-negative double); nullptr: no reduction
    int* flags;                        // [nslices] RDR_FLAG_* bits (OR-reduced)
    const int* nparts_override;        // [nslices][MAX_LEVELS] or nullptr -> ceil(maxlen/max_seg)+1
    int* nslow;                        // [2] number of rays the static classification sent to the generic (slow) kernels; waves of pass 1 that skipped
    int* tile_ctr;                     // [8] per-XCD next-tile counters of this launch (zeroed by the host)
    // pass 1 -> pass 2 workspace (this launch covers tiles [tile_begin, tile_begin + tile_count))
    double* ws; int64_t nslots;
    double* side; int64_t side_cap;    // crossings of the generic rays (compact columns), int* side_ctr = next free column
    int* side_ctr;
    int64_t tile_begin, tile_count;
    const LevelRec* lev;               // [nslices][nz + 1] level records of the light slice loop, written by level_table_kernel BEFORE pass 2 (the march
                                       // kernels read them through the scalar cache and never write them); nullptr: per-ray heights, pass 1
    // outputs
    double* wet; double* hyd;
    // tiling of the whole batch
    int64_t ntiles; int tiles_x;
    int stage_f64;                     // light march on f64 cubes: stage every level's footprint of a wave in LDS (0: the direct gathers)
    int skip_levels;                   // pass 1, lon/lat slice kernels: a wave whose length bounds cannot raise any level maximum leaves the per-level loop
                                       // out (0: never; != 0 only on a launch that allocated skip_smem_bytes); such waves are counted in nslow[1]
    // the one-kernel route (trace_kernel; nullptr on every other call)
    const double* grid_trig;           // (sin, cos) of ypts[ny], then of xpts[nx], in degrees (grid_trig_kernel)
    const int* tile_list;              // pass 1 over a LIST of tiles: walk position lt stands for tile tile_list[lt] of the batch (the probe; reduce only)
    int* one_pass;                     // [OP_WORDS] state of the route (OP_*): trace_kernel reads the snapshot of the probed partition and raises OP_NEED;
                                       // the classic kernels enqueued behind it return at once while OP_NEED is 0
};
// RayParams::one_pass: OP_NEED != 0: the two classic passes must run (a generic ray, a non-finite ray, a partition the probe missed); OP_BITS: what
// fill_partition derives from the PROBED partition (1 poison, 2 clamp_lo, 4 clamp_hi); OP_REDO: calls whose classic passes ran, counted on the
// device; OP_NPARTS: the probed nParts[k]
constexpr int OP_NEED = 0, OP_BITS = 1, OP_REDO = 2, OP_NPARTS = 8, OP_WORDS = OP_NPARTS + MAX_LEVELS;

// The argument block of the two ray kernels as the kernarg segment holds it.  The light instantiations read their uniform parameters from
// there AT THE POINT OF USE, through the constant address space (scalar loads) and a pointer made opaque per site (ray_args): a field
// read this way is a short-lived SGPR next to its use.  Read from the by-value arguments, all of them - some 110 dwords - are kept live
// across the whole tile loop, more than the scalar file holds, and the surplus is parked in lanes of two vector registers: one
// v_readlane_b32 per use, in the vector ALU's issue slots (profiles/r26_tile_body_regs.txt).  What the level loops read as SGPR operands
// stays with the by-value arguments.  Nothing is written through this pointer and the arguments keep arriving as kernel arguments.
template <typename T2> struct RayKernArgs { CubeView<T2> c; RayParams P; LccParams proj; };
static_assert(offsetof(RayKernArgs<float2>, P) == sizeof(CubeView<float2>) && offsetof(RayKernArgs<float2>, proj) == sizeof(CubeView<float2>) + sizeof(RayParams) &&
              sizeof(CubeView<float2>) % 8 == 0 && sizeof(CubeView<double2>) == sizeof(CubeView<float2>) && sizeof(RayParams) % 8 == 0,
              "RayKernArgs mirrors the kernarg layout of (CubeView, RayParams, LccParams): consecutive 8-byte aligned structs");
template <typename T2>
__device__ __forceinline__ const __attribute__((address_space(4))) RayKernArgs<T2>* ray_args() {
    const __attribute__((address_space(4))) RayKernArgs<T2>* p = (const __attribute__((address_space(4))) RayKernArgs<T2>*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));        // (opaque: no load through it is merged with another site's or hoisted out of the tile loop)
    return p;
}

// A tile's records and outputs through scalar bases.  Field f of thread tl of local tile lt is ws[f * nslots + lt * BLOCK + tl]: everything
// but tl is wave-uniform, so the 64-bit part of the address is formed on the scalar unit - base = ws + lt * BLOCK, stepped by nslots per
// field - and the vector part is the thread's constant tl * 8 (< 2 KiB): the access takes the saddr + 32-bit voffset form, no 64-bit vector
// add per field.  No product with nslots ever enters the 32-bit offset (29 * 8 * nslots passes 4 GiB at 19 M rays).
__device__ __forceinline__ int64_t wave_uniform(int64_t v) {                  // v is the same in every lane: as a scalar
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(v >> 32));
    return (int64_t)(((unsigned long long)hi << 32) | lo);
}
typedef __attribute__((address_space(1))) double GlobalF64;       // (the workspace is device memory: global accesses, not flat ones,
typedef __attribute__((address_space(1))) char GlobalByte;        //  also behind a base the compiler cannot look through)
struct TileRecords {
    GlobalByte* base; int64_t fstride; unsigned voff;
    // ws: the workspace (may be null: nothing is accessed then); lt: the tile (wave-uniform); tl: the thread
    __device__ __forceinline__ TileRecords(double* ws, int64_t nslots, int64_t lt, int tl)
        : base((GlobalByte*)(ws + wave_uniform(lt) * BLOCK)), fstride(nslots * (int64_t)sizeof(double)), voff((unsigned)tl * (unsigned)sizeof(double)) {}
    // (each field's base is pinned to scalar registers: left to itself the compiler reassociates the chain of addresses into 64-bit VECTOR
    // multiply-adds, quarter-rate instructions, from one field to the next)
    __device__ __forceinline__ GlobalF64& operator[](int f) const { GlobalByte* b = base + f * fstride; asm("" : "+s"(b)); return *(GlobalF64*)(b + voff); }
    // consecutive fields f, f + 1, ...: one scalar 64-bit add per field
    struct Run {
        GlobalByte* b; int64_t fstride; unsigned voff;
        __device__ __forceinline__ GlobalF64& next() { asm("" : "+s"(b)); GlobalF64& r = *(GlobalF64*)(b + voff); b += fstride; return r; }
    };
    __device__ __forceinline__ Run run(int f) const { return Run{base + f * fstride, fstride, voff}; }
};
static_assert(WS_POLY_LAT == WS_POLY_H + PN && WS_POLY_LON == WS_POLY_LAT + PN && WS_XPOLY == WS_POLY_LON + PN && WS_SCALE == WS_XPOLY + PX && WS_U1 == WS_U0 + 1,
              "the runs of consecutive record fields both passes walk (TileRecords::Run)");

// The slice-uniform level table of build_ray (losreader.py:785-808), computed by one thread into LDS from the LDS z table.
__device__ inline int build_levels(const double2* ez, int nz, double ht, double zref, double* s_lo, double* s_hi, int* s_kz) {
    int K = 0;
    const double ztop = ez[nz - 1].x;
    for (int zz = 0; zz < nz - 1; ++zz) {
        double lo = ez[zz].x, hi = ez[zz + 1].x;
        if (hi == ztop) hi -= 0.01;
        if (hi < ht || lo >= zref) continue;
        if (lo < ht) lo = ht;
        if (hi > zref) hi = zref;
        if (fabs(hi - lo) < 1.0) continue;
        if (K < MAX_LEVELS) { s_lo[K] = lo; s_hi[K] = hi; s_kz[K] = zz; }
        ++K;
    }
    return min(K, MAX_LEVELS);
}

// Per-ray origin heights (RayParams::ht_ray; no reference semantics - DESIGN.md 5c): the reference's level tests
// (losreader.py:785-808) applied with the RAY's height against the slice table built for the lowest one.  Returns the first entry
// k of the table the ray contributes to (K: none) and its clipped bottom lo_i = max(z_kz, hti); every later entry contributes
// unclipped.  Both passes call it with the same inputs.
__device__ __forceinline__ int first_level(const double2* ez, int nz, const double* s_lo, const double* s_hi, const int* s_kz, int K,
                                           double hti, double& lo_i) {
    const double ztop = ez[nz - 1].x;
    // `if high_ht < ht: continue`: the interval tops (before the zref clip) ascend with k, so the entries passing this test are a
    // suffix of the table - found by bisection; (hti NaN: every comparison fails, the search ends at 0 and the ray is NaN anyway)
    int a = 0, b = K;
    while (a < b) {
        const int mid = (a + b) >> 1;
        double hr = ez[s_kz[mid] + 1].x;
        if (hr == ztop) hr -= 0.01;
        if (hr < hti) a = mid + 1; else b = mid;
    }
    for (int k = a; k < K; ++k) {                            // then the first one at least 1 m thick above the ray's own bottom
        const double lo = fmax(s_lo[k], hti);                // `if low_ht < ht: low_ht = ht`
        if (fabs(s_hi[k] - lo) < 1.0) continue;
        lo_i = lo;
        return k;
    }
    lo_i = 0.0;
    return K;
}

// Shared LDS layout of the two ray kernels.  Axis tables are (g[i], 1/(g[i+1]-g[i])) pairs; an x / y axis that is uniform to
// round-off (CubeView::exact_*) needs no table at all (cell_xy works from g0 and the spacing), so the usual lat/lon or LCC grid
// costs 16 B per z level only - a CONUS-sized HRRR grid (1059 x 1799 nodes) would otherwise take 69 KB per workgroup.
// Pass 2's per-level record (slice loop of the light marcher): everything a level needs that is the same for every ray of the slice.
// The records live in a device table (RayParams::lev: per slice nz + 1 of them - the K levels, the weight-0 sentinel behind the last,
// zeros after it), written by level_table_kernel before pass 2 and read by the march kernels with SCALAR loads one level ahead: the
// values are SGPR operands of the fp64 instructions, no vector register, no LDS access and no wait stands in front of a level's gathers.
struct __attribute__((aligned(16))) LevelRec {
    double xv, hs;          // abscissa of the level's top in the crossing polynomial; 0.5e-6/(nParts-1)
    double step, zmid;      // 1/(nParts-1); node g[zb+1] the level's top sits on, zb = window2_base(nz, kz)
    double r0, r1;          // 1/(g[zb+1]-g[zb]), 1/(g[zb+2]-g[zb+1]): the two entries of the top sample's z window
    double gk, rk;          // g[kz], 1/(g[kz+1]-g[kz]): the model interval of the level's interior samples
    int npkz, pad[3];       // nParts | kz << 17
};
static_assert(sizeof(LevelRec) == 80, "LevelRec is the host-visible record of rdr_level_table (include/raider_hip.h)");

struct RaySmem {
    AxisTabs ax;            // axis tables (ey / ex are null for exact axes)
    double2* tab2;          // backing store of the tables
    double* lo; double* hi; // level table
    unsigned long long* mxcol; // [nz][MXCOLS] per-level running maxima of the workgroup, one column per lane%MXCOLS (pass 1)
    double* step;           // [nz] 1/(nParts-1) (pass 2)
    double* hs;             // [nz] 0.5e-6/(nParts-1): half the trapezoid weight per unit of ray length (pass 2)
    double* trig;           // [64] (sin, cos) of the tile's 16 row latitudes, then of its 16 column longitudes (pass 1, GRID rays);
                            // [64..112) LCC cubes: rho of the 16 rows, then (sin, cos) theta of the 16 columns
    double* xv;             // [nz] abscissa of level k's top in the crossing polynomial: (hi[k] - xmap[0]) / xmap[1]
    double* xmap;           // [2] centre and half width of the level-top range hi[1] .. hi[K-1]
    int* kz; int* np; int* K;
};
constexpr int MXCOLS = 16;
__host__ __device__ inline int64_t table_nodes(int64_t ny, int64_t nx, int64_t nz, int exact_y, int exact_x) {
    return (exact_y ? 0 : ny) + (exact_x ? 0 : nx) + nz;
}
__device__ __forceinline__ RaySmem carve_smem(unsigned char* raw, int ny, int nx, int nz, int exact_y, int exact_x) {
    RaySmem m;
    const int nyt = exact_y ? 0 : ny, nxt = exact_x ? 0 : nx;
    m.tab2 = reinterpret_cast<double2*>(raw);                 // 16-byte aligned for ds_read_b128
    m.ax.ey = exact_y ? nullptr : m.tab2;
    m.ax.ex = exact_x ? nullptr : m.tab2 + nyt;
    m.ax.ez = m.tab2 + nyt + nxt;
    m.lo = reinterpret_cast<double*>(m.tab2 + nyt + nxt + nz);
    m.hi = m.lo + nz;
    m.mxcol = reinterpret_cast<unsigned long long*>(m.hi + nz);
    m.step = reinterpret_cast<double*>(m.mxcol + (size_t)nz * MXCOLS);
    m.hs = m.step + nz;
    m.trig = m.hs + nz;
    m.xv = m.trig + 112;
    m.xmap = m.xv + nz;
    m.kz = reinterpret_cast<int*>(m.xmap + 2);
    m.np = m.kz + nz;
    m.K = m.np + nz;
    return m;
}

// bytes carve_smem lays out (the launch's dynamic LDS size) - keep the two in step
inline size_t ray_smem_bytes(int64_t ny, int64_t nx, int64_t nz, int exact_y, int exact_x) {
    return (size_t)table_nodes(ny, nx, nz, exact_y, exact_x) * 16     // axis tables
           + (size_t)nz * 8 * 2                   // lo, hi
           + (size_t)nz * 8 * MXCOLS              // mxcol
           + (size_t)nz * 8 * 2 + 112 * 8         // step, hs, trig
           + (size_t)nz * 8 + 16                  // xv, xmap
           + (size_t)nz * 4 * 2 + 16;             // kz, np, K
}

// Pass 1's two tables BEHIND the common layout - only the launch of a crossings_kernel instantiation that skips (RayParams::skip_levels)
// allocates them, every other ray kernel launches with ray_smem_bytes as it is.  Addressed from m.K afresh wherever they are used (a base kept in a register across the
// polynomial fit is one more value for the allocator to spill):
//   dabs [7][nz]: |xv[k]^n - xv[k-1]^n|, n = 1..7, of the slice's levels k >= 2 (0 below) - the wave bound of a level length;
//   floor [nz]  : the per-level maximum the workgroup had folded into mxcol when it took its current tile (a u64 bit pattern, like mxcol).
__device__ __forceinline__ double* skip_dabs(const RaySmem& m) { return reinterpret_cast<double*>(m.K + 4); }
__device__ __forceinline__ unsigned long long* skip_floor(const RaySmem& m, int nz) { return reinterpret_cast<unsigned long long*>(m.K + 4) + 7 * nz; }
inline size_t skip_smem_bytes(int64_t nz) { return (size_t)nz * 8 * 8; }
// trace_kernel's park BEHIND those two: [PN][BLOCK] doubles, a lane's longitude polynomial while pass 1's folds run (the fit and the folds are the
// register-hungriest stretch, and the march needs the polynomial after them: parked here it is not parked in scratch).  Its launch allocates all three.
__device__ __forceinline__ double* trace_park(const RaySmem& m, int nz) { return reinterpret_cast<double*>(m.K + 4) + 8 * nz; }
inline size_t trace_park_bytes() { return (size_t)PN * BLOCK * 8; }


// Axis tables: once per workgroup.
template <typename T2>
__device__ __forceinline__ void fill_axes(const CubeView<T2>& c, const RaySmem& m) {
    const int tid = threadIdx.x;
    auto fill = [&](double2* dst, const double* g, int n) {
        for (int i = tid; i < n; i += BLOCK) {
            double2 e; e.x = g[i]; e.y = (i == n - 1) ? 0.0 : 1.0 / (g[i + 1] - g[i]);
            dst[i] = e;
        }
    };
    if (m.ax.ey) fill(const_cast<double2*>(m.ax.ey), c.axes, c.ny);
    if (m.ax.ex) fill(const_cast<double2*>(m.ax.ex), c.axes + c.ny, c.nx);
    fill(const_cast<double2*>(m.ax.ez), c.axes + c.ny + c.nx, c.nz);
    __syncthreads();
}

// Level table of one slice (height ht): whenever a workgroup moves on to a tile of another slice.  Called by every thread.
__device__ __forceinline__ int fill_levels(int nz, const RaySmem& m, double ht, double zref) {
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    __syncthreads();                                   // the previous slice's readers are done with the tables
    if (tid == 0) {
        const int K = build_levels(m.ax.ez, nz, ht, zref, m.lo, m.hi, m.kz);
        *m.K = K;
        // range of the level tops the crossing polynomial has to cover (levels 1 .. K-1; level 0 has its own iteration)
        const double a = K > 1 ? m.hi[1] : (K > 0 ? m.hi[0] : 0.0), b = K > 1 ? m.hi[K - 1] : a;
        m.xmap[0] = 0.5 * (a + b);
        m.xmap[1] = fmax(0.5 * (b - a), 1.0);
    }
    __syncthreads();
    const int K = *m.K;
    const double hm = m.xmap[0], ihh = 1.0 / m.xmap[1];
    for (int k = tid; k < K; k += BLOCK) m.xv[k] = (m.hi[k] - hm) * ihh;
    __syncthreads();
    return K;
}

// XCD-aware tile walk: workgroup b runs on XCD b%8 -> each XCD sweeps one contiguous band of tiles (its cube slab stays in
// that XCD's L2).  Within a band the workgroups take tiles from a device counter (one atomic per tile), so no workgroup is
// left holding a fixed share while others have finished.
struct TileWalk {
    int64_t chunk; int xcd; int* ctr; int* slot;
    __device__ __forceinline__ TileWalk(int64_t count, int* counters, int* lds_slot) {
        xcd = blockIdx.x & 7; chunk = (count + 7) / 8; ctr = counters + xcd; slot = lds_slot;
    }
    __device__ __forceinline__ bool next(int64_t count, int64_t& local) {
        __syncthreads();
        if (threadIdx.x == 0) *slot = atomicAdd(ctr, 1);
        __syncthreads();
        const int64_t tt = *slot;
        local = (int64_t)xcd * chunk + tt;
        return tt < chunk && local < count;
    }
};

// Sines / cosines (and, on a conic cube, the origin projection terms) of one of a tile's 16 row latitudes (lane < 16) or 16
// column longitudes, into the tile's LDS table.  (Inlined on purpose: as a real call - tried to keep the libm constants from being
// hoisted and spilled - the kernel returned corrupted slice flags on LCC cubes.)
template <bool LCC>
__device__ __forceinline__ void tile_trig(double v, int lane, const LccParams& proj, double* trig) {
    double sv, cv;
    sincos(v * DEG_TO_RAD, &sv, &cv);
    trig[2 * lane] = sv; trig[2 * lane + 1] = cv;
    if (LCC) {                                             // the origin's projection: per row / per column as well
        if (lane < 16) trig[64 + lane] = lcc_rho(proj, sv, cv);
        else { double st, ct; lcc_theta(proj, v, st, ct); trig[80 + 2 * (lane - 16)] = st; trig[81 + 2 * (lane - 16)] = ct; }
    }
}

// Maximum of a non-negative float over the 64 lanes of a wave, as a wave-uniform value: six DPP steps (within quads, within rows of 16,
// then row 0 -> 1, 2 -> 3 and rows 0-1 -> 2-3) leave it in lane 63.  Non-negative floats order like their bit patterns, so the steps are
// unsigned maxima (v_max_u32 with a DPP operand: one instruction each).  Every lane of the wave must be active.
__device__ __forceinline__ float wave_max_nonneg(float x) {
    unsigned v = (unsigned)__float_as_int(x);
    // (a lane a step leaves out - the rows outside a broadcast's row mask - reads 0, the identity of the unsigned maximum)
#define RDR_DPP_MAX(ctrl, rows) v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, rows, 0xF, false))
    RDR_DPP_MAX(0xB1, 0xF);     // quad_perm [1, 0, 3, 2]
    RDR_DPP_MAX(0x4E, 0xF);     // quad_perm [2, 3, 0, 1]
    RDR_DPP_MAX(0x141, 0xF);    // row_half_mirror
    RDR_DPP_MAX(0x140, 0xF);    // row_mirror
    RDR_DPP_MAX(0x142, 0xA);    // row_bcast:15 into rows 1 and 3
    RDR_DPP_MAX(0x143, 0xC);    // row_bcast:31 into rows 2 and 3
#undef RDR_DPP_MAX
    return __int_as_float(__builtin_amdgcn_readlane((int)v, 63));
}

// A float that is not below |x| (x finite): the product exceeds |x| by 2^-22 |x|, its rounding to float takes back at most 2^-24 |x| -
// or, where the float is subnormal or flushed, at most 2^-126 absolutely, which the caller's absolute margin covers.
__device__ __forceinline__ float float_above_abs(double x) { return (float)(fabs(x) * (1.0 + 0x1p-22)); }

// ---- pass 1: per-ray set-up + level crossings (build_ray, losreader.py:772-835) ------------------------------------
// Optional outputs (both may be on): the per-level batch maximum of the ray length + flags (what delay.py:283,306-311
// reduce over the slice) and the workspace record for pass 2.
// SLOW = false: the light-fp64 path, skips (but counts) the rays the static classification rejects;
// SLOW = true : generic geodesy, processes ONLY those rays, exits at once when there are none.
// LCC (light kernel only): the cube is on a Lambert-conformal-conic grid; a separate instantiation so that the projection's
// pow/tan/sincos code does not weigh on the register allocation of the lon/lat one.
// OM (light kernel only): how the batch is given, fixed at compile time so that the hot instantiations carry none of the libm
// code of the other input forms (atan / atan2 of XYZ origins, four sincos of inc/heading look vectors) - with everything in one
// body the compiler hoisted so many of their invariants that the per-level loop spilled (220 B of scratch per lane in round 1):
//   1: GRID origins + per-pixel look vectors;  2: GRID origins + incidence / heading (arrays or scalars) or zenith;  0: any.
// PR (light kernel only): per-ray origin heights (P.ht_ray) - a separate instantiation so that the slice kernels carry none of it; the
// generic kernel looks at P.ht_ray at run time.
// (pass 2's pieces the TRACE body calls; defined with pass 2 below)
template <typename T2, int E, bool NC>
__device__ __forceinline__ void march_slice_levels(const CubeView<T2>& c, const EpochCubes<T2, E>& ev, const RaySmem& m, const RayPoly& q, const double (&xc)[PX],
                                                   const LevelRec* lev, double u0, double u1, int K, bool clamp_lo, bool clamp_hi, unsigned long long live,
                                                   double* acc_w, double* acc_h);
__device__ __forceinline__ bool lane_nocheck(double u0r, double u1r, bool active, bool mine, RayPoly& q, double (&xc)[PX], int ny, int nx);
template <typename RP>
__device__ __forceinline__ void tile_ray(const RP& P, int64_t t, int tl, int64_t& i, bool& active);
// TRACE (trace_kernel; lon/lat f32 slice rays on a REGULAR cube): the tile's rays are marched where they were fitted, from registers, on the
// PROBED partition - pass 1 as it stands (same set-up, same fit, same folds: the body is written once, so the bits of q, xc, u0, u1 and scale
// cannot differ from the records' of the two-pass route), then march_slice_levels as march_kernel calls it.  No record is written or read.
template <typename T2, bool SLOW, bool LCC, int OM, bool PR, bool TRACE>
__device__ __forceinline__ void pass1_tiles(const CubeView<T2>& c, const RayParams& P, const LccParams& proj) {
    static_assert(!SLOW || (OM == 0 && !PR), "the generic kernel takes every input form");
    static_assert(!TRACE || (!SLOW && !LCC && !PR && OM != 0), "the one-kernel route: light lon/lat slice rays of a GRID batch");
    if (!TRACE && P.one_pass != nullptr && P.one_pass[OP_NEED] == 0) return;       // (enqueued behind trace_kernel, which needed no second opinion)
    const bool per_ray = PR || (SLOW && P.ht_ray != nullptr);
    if (SLOW && *P.nslow == 0) return;
    // The uniform parameters as the tile loop reads them: the light instantiations through the kernarg segment, afresh at every site
    // (RayKernArgs); the generic kernel from its by-value arguments.
    auto Pk = [&]() -> decltype(auto) { if constexpr (SLOW) return (P); else return (ray_args<T2>()->P); };
    auto Ck = [&]() -> decltype(auto) { if constexpr (SLOW) return (c); else return (ray_args<T2>()->c); };
    auto Jk = [&]() -> decltype(auto) { if constexpr (SLOW) return (proj); else return (ray_args<T2>()->proj); };
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const RaySmem m = carve_smem(smem_raw, c.ny, c.nx, c.nz, c.exact_y, c.exact_x);
    // TRACE: the cube view of the march (march_kernel's REGULAR), and what the probed partition decides for every ray (OP_BITS)
    CubeView<T2> cm = c;
    if (TRACE) { cm.exact_y = 1; cm.exact_x = 1; cm.small = 1; }
    double poison = 0.0;
    bool clamp_lo = false, clamp_hi = false;
    // The instantiations whose waves may skip the per-level length loop (below): not the per-ray-height ones (their loop starts per lane), and
    // not on conic cubes (those spill around the fit already, and the decision added 8 to 16 B of scratch to them).
    constexpr bool SKIPPABLE = !SLOW && !PR && !LCC;
    if (SKIPPABLE && threadIdx.x == 0) m.K[3] = 0;        // the workgroup's count of waves that skipped (before the barrier of fill_axes)
    fill_axes(c, m);
    const int tid = threadIdx.x;
    // (kernel-uniform; read afresh at every use, so that no flag of them is carried across the tile body)
    auto reduce_on = [&]() { return Pk().maxlen_bits != nullptr; };
    auto skip_on = [&]() { if (!SKIPPABLE) return false; const auto& a = Pk(); return a.maxlen_bits != nullptr && a.skip_levels != 0; };
    // per-level maximum of the ray length over a slice (delay.py:283): every lane folds its length into column lane%16 of
    // the workgroup's LDS table with one ds_max_u64 (non-negative doubles order like their bit patterns); the columns are
    // combined when the workgroup leaves the slice (flush).  NaN lengths are left out here and reported through the flags,
    // which is how ndarray.max's NaN poisoning is reproduced on the host side.
    int my_flags = 0;
    int K = 0, slice = -1;
    double ht = P.ht;
    auto flush = [&]() {                                   // called by every thread of the workgroup
        const auto& a = Pk();
        if (a.maxlen_bits == nullptr || slice < 0) return;
        __syncthreads();
        int tf = threadIdx.x;
        asm volatile("" : "+v"(tf));                       // (opaque: no address derived from it is kept live across the tile loop)
        for (int k = tf; k < K; k += BLOCK) {
            unsigned long long v = 0ULL;
#pragma unroll
            for (int cc = 0; cc < MXCOLS; ++cc) v = max(v, m.mxcol[k * MXCOLS + cc]);
            atomicMax(&a.maxlen_bits[(int64_t)slice * MAX_LEVELS + k], v);
        }
        int f = my_flags;
        for (int off = 32; off > 0; off >>= 1) f |= __shfl_xor(f, off, 64);
        if ((tf & 63) == 0 && f) atomicOr(a.flags + slice, f);
        my_flags = 0;
    };
    TileWalk walk(P.tile_count, P.tile_ctr, m.K + 2);
    int64_t lt;
    while (walk.next(Pk().tile_count, lt)) {
        const auto& pa = Pk();                             // (this site: the tile's place in the batch and its rays)
        const int origin_mode = OM != 0 ? 0 : pa.origin_mode;
        const int los_mode = OM == 1 ? 0 : pa.los_mode;
        const int64_t tg = pa.tile_list ? (int64_t)pa.tile_list[lt] : pa.tile_begin + lt;   // tile of the batch; t: tile within its slice
        const int sl = (int)(tg / pa.tiles_per_slice);
        const int64_t t = tg - (int64_t)sl * pa.tiles_per_slice;
        if (sl != slice) {                                 // (workgroup-uniform) first tile, or the walk has reached the next slice
            flush();
            slice = sl;
            ht = pa.hts ? pa.hts[sl] : pa.ht;
            K = fill_levels(Ck().nz, m, ht, pa.zref);
            int tz = threadIdx.x;
            asm volatile("" : "+v"(tz));
            if constexpr (TRACE) {
                // the columns start from the PROBED maxima (column 0; any value the device table has held is a maximum of the slice): the floor
                // of the skip decisions below then stands near the final maxima from the first tile on, and almost every wave takes level 1 only
                for (int k = tz; k < K * MXCOLS; k += BLOCK)
                    m.mxcol[k] = (k & (MXCOLS - 1)) == 0 ? pa.maxlen_bits[(int64_t)sl * MAX_LEVELS + (k / MXCOLS)] : 0ULL;
                const int bits = pa.one_pass[OP_BITS];
                poison = (bits & 1) ? qnan() : 0.0; clamp_lo = (bits & 2) != 0; clamp_hi = (bits & 4) != 0;
            } else
            if (reduce_on()) for (int k = tz; k < K * MXCOLS; k += BLOCK) m.mxcol[k] = 0ULL;
            if (skip_on()) {
                double* const dabs = skip_dabs(m);
                const int nz = Ck().nz;
                unsigned long long* const flr = skip_floor(m, nz);
                // the slice's table of the wave bound (below): |v_k^n - v_(k-1)^n| for the levels the bound is used for, and a floor of 0
                for (int k = tz; k < K; k += BLOCK) {
                    const double v1 = m.xv[k], v0 = k >= 2 ? m.xv[k - 1] : v1;
                    double p1 = v1, p0 = v0;
#pragma unroll
                    for (int n = 0; n < 7; ++n) { dabs[n * nz + k] = fabs(p1 - p0); p1 *= v1; p0 *= v0; }
                    flr[k] = 0ULL;
                }
            }
            __syncthreads();
        }
        if (skip_on()) {
            unsigned long long* const flr = skip_floor(m, Ck().nz);
            // the floor of this tile's skip decisions: what the workgroup's earlier tiles have folded into the columns (the barriers of
            // walk.next() are behind us).  It only ever trails the columns, and a stale floor merely skips less.  GRID origins have the
            // barrier of the tile's sines / cosines between this store and the decisions that read it; list origins have none: a wave
            // that is ahead may read an entry before or after its refresh.  That is sound because either value is a maximum the columns
            // have held in THIS slice (the slice change zeroes the floor before its own barrier) and an aligned 64-bit LDS store is one
            // ds_write_b64, which does not tear.
            int tf = threadIdx.x;
            asm volatile("" : "+v"(tf));
            for (int k = tf; k < K; k += BLOCK) {
                unsigned long long v = 0ULL;
#pragma unroll
                for (int cc = 0; cc < MXCOLS; ++cc) v = max(v, m.mxcol[k * MXCOLS + cc]);
                flr[k] = v;
            }
        }
        // The thread index as the tile body sees it: an opaque per-tile copy, so that nothing derived from it (LDS addresses, record
        // pointers, row / column offsets) is hoisted out of the tile loop and kept live - or spilled - across the polynomial fit.
        int tl = threadIdx.x;
        asm volatile("" : "+v"(tl));
        int64_t i, row = 0, col = 0; bool active;
        if (origin_mode == 0) {
            const int64_t ty = t / pa.tiles_x, tx = t - ty * pa.tiles_x;
            row = ty * TILE + (tl >> 4); col = tx * TILE + (tl & 15);
            active = row < pa.ny && col < pa.nx;
            i = row * pa.nx + col;
        } else {
            i = t * BLOCK + tl;
            active = i < pa.n;
        }
        // ---- origin: llh -> ECEF (delay.py:262-267)
        double lat = 0, lon = 0, ox = qnan(), oy = qnan(), oz = qnan();
        double hti = ht;                                   // the ray's origin height: the slice's, or its own
        if (PR || SLOW) { if (per_ray && active) hti = pa.ht_ray[i]; }
        RayBase base;
        if (!SLOW && origin_mode == 0) {
            if constexpr (TRACE) {
                if (active) { lat = pa.ypts[row]; lon = pa.xpts[col]; }
                base.lat0 = lat; base.lon0 = lon;
                // the same sines / cosines, from the table grid_trig_kernel filled with the same call (RayParams::grid_trig): with sincos in
                // this kernel its constants are hoisted out of the tile loop, 20 registers the march does not have
                base.s0 = 0.0; base.c0 = 1.0; base.sl0 = 0.0; base.cl0 = 1.0;
                if (active) {
                    const double* const gy = pa.grid_trig + 2 * row; const double* const gx = pa.grid_trig + 2 * (pa.ny + col);
                    base.s0 = gy[0]; base.c0 = gy[1]; base.sl0 = gx[0]; base.cl0 = gx[1];
                }
            } else {
            // a tile has 16 distinct latitudes and 16 distinct longitudes: 32 lanes take the sines / cosines for everybody
            // (the previous tile's readers are past the barriers of walk.next())
            if (tl < 32) {
                const int64_t ty = t / pa.tiles_x, tx = t - ty * pa.tiles_x;
                const int64_t r = ty * TILE + (tl & 15), cc = tx * TILE + (tl & 15);
                const double v = tl < 16 ? (r < pa.ny ? pa.ypts[r] : 0.0) : (cc < pa.nx ? pa.xpts[cc] : 0.0);
                tile_trig<LCC>(v, tl, proj, m.trig);
            }
            __syncthreads();
            if (active) { lat = pa.ypts[row]; lon = pa.xpts[col]; }
            base.lat0 = lat; base.lon0 = lon;
            base.s0 = active ? m.trig[2 * (tl >> 4)] : 0.0; base.c0 = active ? m.trig[2 * (tl >> 4) + 1] : 1.0;
            base.sl0 = active ? m.trig[32 + 2 * (tl & 15)] : 0.0; base.cl0 = active ? m.trig[33 + 2 * (tl & 15)] : 1.0;
            }
            if (active) {                                          // lla2ecef (geodesy.h) with the shared sines / cosines
                const double N = WGS84_A / sqrt(1.0 - WGS84_ES * base.s0 * base.s0);
                ox = (N + hti) * base.c0 * base.cl0;
                oy = (N + hti) * base.c0 * base.sl0;
                oz = (N * (1.0 - WGS84_ES) + hti) * base.s0;
            }
        } else {
            if (active) {
                if (origin_mode == 0) { lat = pa.ypts[row]; lon = pa.xpts[col]; }
                else if (pa.lat) { lat = pa.lat[i]; lon = pa.lon[i]; }
                if (origin_mode == 2) {
                    ox = pa.xyz[3 * i]; oy = pa.xyz[3 * i + 1]; oz = pa.xyz[3 * i + 2];
                    if (!pa.lat) { double h0_; ecef2lla(ox, oy, oz, lon, lat, h0_); }   // frame for the delta lat/lon formulas
                } else lla2ecef(lat, lon, hti, ox, oy, oz);
            }
            base = make_base(lat, lon);
        }
        // ---- look vector (delay.py:270)
        double lx = qnan(), ly = qnan(), lz = qnan();
        if (active) {
            const auto& la = Pk();                         // (this site: the look vectors)
            const int64_t lbase = (int64_t)sl * la.los_stride;  // this slice's block of the look-vector / incidence arrays
            // (inc / heading: the origin's own sines / cosines are the ones inc_hd_to_ecef would compute again)
            if (los_mode == 0) { const double* lp = la.los + 3 * (lbase + i); lx = lp[0]; ly = lp[1]; lz = lp[2]; }
            else if (los_mode == 1) inc_hd_to_ecef_sc(la.inc[lbase + i], la.hd ? la.hd[lbase + i] : la.hd0, base.s0, base.c0, base.sl0, base.cl0, lx, ly, lz);
            else if (los_mode == 2) inc_hd_to_ecef_sc(la.inc0, la.hd0, base.s0, base.c0, base.sl0, base.cl0, lx, ly, lz);
            else { lx = base.c0 * base.cl0; ly = base.c0 * base.sl0; lz = base.s0; }   // zenith (losreader.py:302-316)
        }
        // |l| (1 for unit look vectors): ray length between two crossings = (t_hi - t_lo) * |l|   (losreader.py:821)
        const double nl2 = fma(lx, lx, fma(ly, ly, lz * lz));
        const double nl = nl2 * rsq_nr<2>(nl2);
        // Static classification: may the ray polynomials be used along the WHOLE ray?  gam bounds the angular travel
        // (t_max <= (zref-ht)/cos(inc) because the local zenith angle of a straight ray decreases with height); the ray must
        // stay clear of the poles (cos(lat) > gam + 0.02), turn by less than 0.12 rad in longitude (gam / (cos(lat) - gam)) and
        // be shorter than 0.035 rad - inside that region the degree-5 interpolants are good to 2.5e-7 m in height and, on the
        // ground, to 5.9e-5 m (lat) and 1.5e-4 m (lon) at worst, 3.1e-5 m and 9.4e-5 m on rays shorter than 100 km
        // (tests/test_ray_poly_bounds.py).  The longitude limit is set by what that interpolation error does to a delay: a field
        // LINEAR in longitude with the strongest horizontal gradient of the synthetic cube (62 N-units per degree at 75-80 deg N)
        // held through a whole 41 km column moves a delay by 8.8e-10 m at 70 deg incidence, under the 1e-9 m of the parity suites;
        // at 0.2 rad, the limit before, it was 3.9e-9 m (tests/test_gpu_ray_geometry.py, which measures this part apart from the
        // offset of the level crossings against the reference's height: that one does not depend on the classification).
        // The ray must not reach the +-180 meridian either (the light path does not wrap longitudes).
        const double cosi = (lx * base.c0 * base.cl0 + ly * base.c0 * base.sl0 + lz * base.s0) / nl;
        const double zref = Pk().zref;
        const double gam = (zref - hti) / (cosi * 6.3e6);
        // LCC cubes: spherical cones only (HRRR), and the node projections use short series in log(t/t_origin) <= gam / cos(lat)
        // (geodesy_fast.h); an ellipsoidal cone goes to the generic kernels (lcc_forward) ray by ray.
        // The +-180 deg meridian: the light path carries longitude UNWRAPPED (origin + small delta), the reference wraps every
        // sample into (-180, 180] (atan2).  The two agree whenever no sample crosses the meridian (origin more than 5 deg away from
        // it - a ray travels < 0.12 rad = 6.9 deg only at high latitude, where the other clauses bite first... kept as before), and
        // ALSO when a crossing sample is outside the cube either way: a lon/lat cube whose x axis ends at or before +180 and starts
        // more than 12 deg after -180 (wrap_pos) gives NaN for an unwrapped 180.x (beyond the axis) and for the reference's
        // wrapped -179.x (before it) alike; mirrored for origins near -180 (wrap_neg).  Dateline scenes (Fiji, Chukotka, the
        // Aleutians) then stay on the light path.  On a conic / polar-stereographic cube only the cone's own cut meridian
        // lam0 +- 180 matters (theta = n (lam - lam0) is wrapped there); geographic +-180 is an ordinary meridian.
        bool lon_ok;
        const auto& ja = Jk();
        const int proj_kind = ja.kind;
        if (proj_kind == 1) {
            double dl = lon - ja.lam0 * RAD_TO_DEG;
            dl -= 360.0 * rint(dl * (1.0 / 360.0));
            lon_ok = fabs(dl) + 12.0 < 180.0;
        } else {
            const auto& ca = Ck();
            const double x_lo = ca.x_lo, x_hi = ca.x_hi;
            const bool wrap_pos = (x_hi <= 180.0) & (x_lo > -168.0), wrap_neg = (x_lo >= -180.0) & (x_hi < 168.0);
            lon_ok = (fabs(lon) + 5.0 < 180.0) || ((fabs(lon) <= 180.0) && (lon > 0.0 ? wrap_pos : wrap_neg));
        }
        const bool fast_ok = !active || ((cosi > 0.05) && (base.c0 > gam + 0.02) && (gam < 0.12 * (base.c0 - gam)) && (gam < 0.035) &&
                                         lon_ok && (proj_kind != 1 || (ja.e == 0.0 && gam < 0.09 * base.c0)));   // (run-time test: the generic kernels must classify identically)
        if (!SLOW) {
            const unsigned long long slow_mask = __ballot(!fast_ok);
            if (slow_mask && (tl & 63) == 0) atomicAdd(Pk().nslow, (int)__popcll(slow_mask));
            if constexpr (TRACE) { if (slow_mask && (tl & 63) == 0) atomicOr(Pk().one_pass + OP_NEED, 1); }   // a ray for the generic kernels
        }
        const bool mine = SLOW ? !fast_ok : fast_ok;      // lanes this instantiation is responsible for
        if (SLOW && !__any(mine)) continue;               // (wave-uniform) nothing to mop up in this wave
        // per-ray heights: the ray's first level of the slice table and that level's clipped bottom (k0 == K: no level at all -
        // the ray counts for nothing and its delays are 0, as a slice without levels).  A height below the table's is a caller
        // error (flag 32: the slice's outputs are NaN).
        int k0 = 0; double lo_first = K > 0 ? m.lo[0] : 0.0;
        if (PR || SLOW) {
            if (per_ray) {
                k0 = first_level(m.ax.ez, Ck().nz, m.lo, m.hi, m.kz, K, hti, lo_first);
                if (active && mine && hti < ht) my_flags |= 32;
            }
        }
        const bool cnt = active && mine && k0 < K;
        // this lane's column of the per-level maxima; derived afresh per tile (an address kept live across the polynomial fit,
        // the register-hungriest stretch of the kernel, is the one value the allocator had to spill)
        int mxcol_idx = tl & (MXCOLS - 1);
        asm volatile("" : "+v"(mxcol_idx));
        unsigned long long* const mxc = m.mxcol + mxcol_idx;
        if constexpr (SLOW) {
            double* const w = P.ws ? P.ws + (lt * BLOCK + tl) : nullptr;
            const int64_t ns = P.nslots;
            const bool reduce = reduce_on();
            // a column of the side buffer for this ray's K+1 crossings: one device atomic per wave, columns handed out in lane
            // order; -1 when the buffer is full (pass 2 then recomputes the crossings)
            int64_t sidx = -1;
            if (w) {
                const unsigned long long mm = __ballot(mine);
                const int lane = tl & 63;
                int base = 0;
                if (lane == 0) base = atomicAdd(P.side_ctr, (int)__popcll(mm));
                base = __shfl(base, 0, 64);
                const int64_t cand = (int64_t)base + __popcll(mm & ((1ULL << lane) - 1ULL));
                if (mine && cand < P.side_cap) sidx = cand;
            }
            double* const sd = (sidx >= 0) ? P.side + sidx : nullptr;
            if (w && mine) {
                w[(int64_t)WS_SCALE * ns] = 0.0;
                w[(int64_t)(WS_ORIGIN + 0) * ns] = ox; w[(int64_t)(WS_ORIGIN + 1) * ns] = oy; w[(int64_t)(WS_ORIGIN + 2) * ns] = oz;
                w[(int64_t)(WS_LOS + 0) * ns] = lx; w[(int64_t)(WS_LOS + 1) * ns] = ly; w[(int64_t)(WS_LOS + 2) * ns] = lz;
                w[(int64_t)WS_LAT0 * ns] = lat; w[(int64_t)WS_LON0 * ns] = lon;
                w[(int64_t)WS_S0 * ns] = base.s0; w[(int64_t)WS_C0 * ns] = base.c0;
                w[(int64_t)WS_SL0 * ns] = base.sl0; w[(int64_t)WS_CL0 * ns] = base.cl0;
                w[(int64_t)WS_SIDE * ns] = (double)sidx;
            }
            double t_hi = 0.0, inv_cosf = 1.0;
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                if (k < k0) continue;                // (per-ray heights: the ray joins the slice's level table at k0)
                const double lo = k == k0 ? lo_first : m.lo[k], hi = m.hi[k];
                // first interval: cos_factor is None -> 10 iterations with factor 1 for both ends (losreader.py:812-825);
                // later intervals reuse the previous top as their bottom (losreader.py:811-812)
                double t_lo = t_hi;
                if (k == k0) t_lo = toa_newton_t(ox, oy, oz, lx, ly, lz, lo, 10, 1.0);
                t_hi = toa_newton_t(ox, oy, oz, lx, ly, lz, hi, k == k0 ? 10 : 3, inv_cosf);
                const double L = fabs(t_hi - t_lo) * nl;                                   // np.linalg.norm(high - low) (losreader.py:821): positive also for the
                                                                                            // reversed segment of an origin ABOVE zref inside zref's model interval
                if (k == k0) inv_cosf = L / (hi - lo);                                      // 1/cos_factor, losreader.py:824-825
                if (sd) {
                    if (k == k0) sd[0] = t_lo;
                    sd[(int64_t)(k + 1) * P.side_cap] = t_hi;
                }
                if (reduce) {
                    if (cnt) my_flags |= (L != L) ? 1 : 2;
                    atomicMax(&mxc[k * MXCOLS], (unsigned long long)__double_as_longlong((cnt && L > 0.0) ? L : 0.0));
                    if (k == k0 && cnt) {            // first sample of the ray (fraction 0)
                        const double h0 = ecef_height(fma(t_lo, lx, ox), fma(t_lo, ly, oy), fma(t_lo, lz, oz));
                        if (!(h0 < c.z_lo)) my_flags |= 4;
                    }
                    if (k == K - 1 && cnt) {         // last sample of the ray (fraction 1)
                        const double h1 = ecef_height(fma(t_hi, lx, ox), fma(t_hi, ly, oy), fma(t_hi, lz, oz));
                        if (!(h1 > c.z_hi)) my_flags |= 8;
                    }
                }
            }
        } else {
            // ---- light rays: fit h(u), lat(u), lon(u) once, then everything is polynomial arithmetic.
            // Range of the ray parameter any Newton iterate / sample can take: iterates start at t0 = level height
            // (>= ht) and move monotonically to the crossing, which lies in [0, (zref - ht)/cos(inc)].
            // (an origin ABOVE zref inside zref's model interval - the reference's one reversed segment, low_ht = ht > high_ht = zref - starts its
            // iterates at t0 = ht and ends them at a NEGATIVE ray parameter: both belong to the range.  Unchanged for ht <= zref.)
            const double t_end = (zref - hti) / (cosi * nl);
            const double t_a = fmin(fmin(0.0, hti), t_end) - 1.0;
            const double t_b = fmax(fmax(zref, hti), t_end) + 1.0;
            const double half = 0.5 * (t_b - t_a), mid = 0.5 * (t_b + t_a);
            const double su = 1.0 / half, ou = -mid * su;
            RayPoly q;
            LccOrigin lorg = {0.0, 0.0, 0.0};
            const bool shared_lcc = LCC && !SLOW && origin_mode == 0;
            if (shared_lcc) { lorg.rho = m.trig[64 + (tl >> 4)]; lorg.st = m.trig[80 + 2 * (tl & 15)]; lorg.ct = m.trig[81 + 2 * (tl & 15)]; }
            fit_ray_poly<LCC>(base, ox, oy, oz, lx, ly, lz, mid, half, proj, shared_lcc ? &lorg : nullptr, q);
            const double scale = nl * half;                           // ray length per unit of u
            // The record's stores (TileRecords), at each of the three places they stand; the base is formed afresh each time.
            auto records = [&]() { const auto& a = Pk(); return TileRecords(a.ws, a.nslots, lt, tl); };
            auto has_ws = [&]() { if constexpr (TRACE) return false; else return Pk().ws != nullptr; };
            if (TRACE || (has_ws() && mine)) {
                // exact-uniform axes: hand pass 2 the INDEX-space coordinate (v - g0) * (n-1)/(g[n-1]-g0) directly (cell_xy<true>)
                const auto& ca = Ck();
                if (ca.exact_y) {
                    const double inv_dy = ca.inv_dy;
                    q.lat[0] = (q.lat[0] - ca.y_lo) * inv_dy;
#pragma unroll
                    for (int n = 1; n < PN; ++n) q.lat[n] *= inv_dy;
                }
                if (ca.exact_x) {
                    const double inv_dx = ca.inv_dx;
                    q.lon[0] = (q.lon[0] - ca.x_lo) * inv_dx;
#pragma unroll
                    for (int n = 1; n < PN; ++n) q.lon[n] *= inv_dx;
                }
                if constexpr (TRACE) {
                    double* const park = trace_park(m, ca.nz) + tl;
#pragma unroll
                    for (int n = 0; n < PN; ++n) park[n * BLOCK] = q.lon[n];
                } else {
                    const TileRecords w = records();
                    TileRecords::Run r = w.run(WS_POLY_H);
#pragma unroll
                    for (int n = 0; n < PN; ++n) r.next() = q.h[n];
#pragma unroll
                    for (int n = 0; n < PN; ++n) r.next() = q.lat[n];
#pragma unroll
                    for (int n = 0; n < PN; ++n) r.next() = q.lon[n];
                    w[WS_SCALE] = scale;
                }
            }
            // getTopOfAtmosphere carried on u: u0 = u(h); u += (h - H(u)) * su / factor   (losreader.py:724-731)
            // Level 0 (ten plain Newton steps per end, losreader.py:770-777) sets the gain of every later level.
            double u_hi = 0.0, gain = su;
            double u_first = 0.0;       // (TRACE: the bottom crossing of the first level, field WS_U0 of a record)
            double last_len = 0.0;      // a light ray's lengths are NaN for every level or for none (they all stem from one polynomial)
            if (PR ? (k0 < K) : (K > 0)) {
                const double lo = PR ? lo_first : m.lo[0], hi = PR ? m.hi[k0] : m.hi[0];
                double u_lo = fma(lo, su, ou);
                u_hi = fma(hi, su, ou);
#pragma unroll 1
                for (int it = 0; it < 10; ++it) {
                    u_lo = fma(lo - poly5(q.h, u_lo), su, u_lo);
                    u_hi = fma(hi - poly5(q.h, u_hi), su, u_hi);
                }
                const double L = fabs(u_hi - u_lo) * scale;                                    // a norm (losreader.py:821): an origin above zref in zref's own model
                                                                                               // interval gives ONE reversed segment (low_ht = ht > high_ht = zref) of positive length
                last_len = L;
                gain = su * (L / (hi - lo));                                                   // su / cos_factor, losreader.py:824-825
                if (has_ws() && mine) { TileRecords::Run r = records().run(WS_U0); r.next() = u_lo; r.next() = u_hi; }
                if constexpr (TRACE) u_first = u_lo;
                if (reduce_on()) {
                    atomicMax(&mxc[PR ? k0 * MXCOLS : 0], (unsigned long long)__double_as_longlong((cnt && L > 0.0) ? L : 0.0));
                    if (cnt && !(poly5(q.h, u_lo) < Ck().z_lo)) my_flags |= 4;                    // first sample of the ray
                }
            }
            // Later levels: the three-iteration crossing as a polynomial of the level height (fit_crossing_poly)
            double xc[PX];
            fit_crossing_poly(q.h, su, ou, gain, m.xmap[0], m.xmap[1], xc);
            if (has_ws() && mine) {
                TileRecords::Run r = records().run(WS_XPOLY);
#pragma unroll
                for (int n = 0; n < PX; ++n) r.next() = xc[n];
            }
            const bool reduce = reduce_on();
            if (reduce) {
                // The level abscissae are read from LDS ahead of the ds_max of the previous pair: LDS operations complete in
                // order, so a read issued after an atomic would wait for it.
                // A lane that does not count (tile padding, a ray left to the generic kernel) contributes length 0 to every
                // level: its scale is zeroed once, here, instead of a select per level; v_max_f64(L, 0) then also maps a NaN
                // length (0 x NaN of such a lane, or a genuinely NaN ray - reported through the flags) to 0, so that the u64
                // maximum never sees a negative or non-finite bit pattern.
                // The metres-per-unit-u scale is folded into the polynomial once (8 multiplications), so a level costs 7 FMAs, one
                // subtraction and the v_max.
                const double mscale = cnt ? scale : 0.0;
                // the ray's last crossing (flags below); TRACE keeps xc for the march and takes it behind the loops, one value less across them
                auto last_crossing = [&]() { return (PR ? (k0 + 1 < K) : (K > 1)) ? poly7(xc, m.xv[K - 1]) : u_hi; };
                double u_end = 0.0;
                if constexpr (!TRACE) u_end = last_crossing();
                double xm[PX];
#pragma unroll
                for (int n = 0; n < PX; ++n) xm[n] = xc[n] * mscale;
                double s_hi = u_hi * mscale;                                                   // scaled crossing of the previous level
                int k = 1;
                if constexpr (PR) {
                    // per-ray heights: levels up to the ray's own first one (k <= k0) count 0; level k0 + 1 starts from the
                    // ten-iteration crossing u_hi of level k0, as level 1 of a slice does
                    const double s_first = s_hi;
                    for (; k < K; ++k) {
                        const double st = poly7(xm, m.xv[k]);
                        const double L = st - (k == k0 + 1 ? s_first : s_hi);
                        s_hi = st;
                        atomicMax(&mxc[k * MXCOLS], (unsigned long long)__double_as_longlong(k > k0 ? fmax(fabs(L), 0.0) : 0.0));
                    }
                }
                // Can this wave raise any level maximum at all?  Most cannot: the lengths go with the secant of the incidence angle, and
                // after a few tiles the workgroup's columns hold the lengths of rays near the far edge of the swath.  A level k >= 2 has
                //   L_k = |X(v_k) - X(v_(k-1))|,  X(v) = sum xm[n] v^n   =>   L_k <= sum_{n>=1} |xm[n]| |v_k^n - v_(k-1)^n|
                // for every ray, hence  L_k <= sum_{n>=1} A[n] Dabs[n][k]  with A[n] the wave's maximum of |xm[n]| over the lanes that count (the
                // others enter as 0 - their xm is 0, or NaN under tile padding, and the loop folds 0 for them either way) and Dabs the slice's table.  The COMPUTED length may exceed the exact one by the rounding of the two Horner
                // chains, each within 8 ulp of sum_{n>=0} |xm[n]| |v|^n <= S = sum |xm[n]| (|v| <= 1 from level 1 on): 2^-49 S with the
                // subtraction's own rounding; the table entries carry 2^-49 absolutely (six products each side, one subtraction), which
                // the A[n] multiply to at most 7 x 2^-49 max(S); the float maxima are rounded up
                // (float_above_abs) short of 2^-122 in all, and the seven-term sum of the bound rounds by
                // a few ulp relatively.  B_k = (1 + 2^-30) sum A[n] Dabs[n][k] + 2^-44 max(S) + 2^-120 covers all of it with room to spare,
                // and both margins are far below the difference between two neighbouring columns of a scene.  If B_k <= floor[k] for every
                // level - an equal value does not change a maximum - nothing this wave computes in the loop below can change a column.
                // Level 1 starts from the ten-iteration crossing of level 0, which is not a value of X: it is always computed.  A NaN
                // or infinite coefficient of a lane that counts (S not finite) takes the loop.  One decision per wave and tile; lane j bounds levels j and j + 64.
                bool skip = false;
                if constexpr (SKIPPABLE) {
                    if (K > 2 && K <= 128 && skip_on()) {
                        const int nz = Ck().nz;
                        const double* const dabs = skip_dabs(m);
                        const unsigned long long* const flr = skip_floor(m, nz);
                        double S = fabs(xm[0]);
#pragma unroll
                        for (int n = 1; n < PX; ++n) S += fabs(xm[n]);
                        if (!cnt) S = 0.0;
                        const bool finite = !__any(!(S < __builtin_inf()));
                        if constexpr (TRACE) { if (!finite && (tl & 63) == 0) atomicOr(Pk().one_pass + OP_NEED, 1); }   // a NaN or infinite ray
                        const float a0 = wave_max_nonneg(finite ? float_above_abs(S) : 0.0f);
                        if (finite && a0 == 0.0f) skip = true;                                 // nothing but lanes that do not count
                        else if (finite) {
                            const int lane = tl & 63;
                            const int ka = min(lane, K - 1), kb = min(lane + 64, K - 1);
                            double Ba = 0.0, Bb = 0.0;
#pragma unroll
                            for (int n = 1; n < PX; ++n) {
                                const double an = (double)wave_max_nonneg(cnt ? float_above_abs(xm[n]) : 0.0f);
                                Ba = fma(an, dabs[(n - 1) * nz + ka], Ba);
                                if (K > 64) Bb = fma(an, dabs[(n - 1) * nz + kb], Bb);
                            }
                            // (TRACE holds the lat / lon polynomials through this stretch.  Left alone, the two sums are sunk into the branch of
                            // the lanes that compare them, and the seven maxima and table entries wait there side by side - in scratch)
                            if constexpr (TRACE) asm volatile("" : "+v"(Ba), "+v"(Bb));
                            const double margin = fma((double)a0, 0x1p-44, 0x1p-120);
                            Ba = fma(Ba, 1.0 + 0x1p-30, margin);
                            Bb = fma(Bb, 1.0 + 0x1p-30, margin);
                            bool ok = lane < 2 || lane >= K || (unsigned long long)__double_as_longlong(Ba) <= flr[ka];
                            if (K > 64) ok = ok && (lane + 64 >= K || (unsigned long long)__double_as_longlong(Bb) <= flr[kb]);
                            skip = !__any(!ok);
                            if (skip && lane == 0) atomicAdd(m.K + 3, 1);                      // (diagnostics: rdr_skipped_wave_count)
                        }
                    }
                }
                if (skip) {
                    const double L = poly7(xm, m.xv[1]) - s_hi;
                    atomicMax(&mxc[MXCOLS], (unsigned long long)__double_as_longlong(fmax(fabs(L), 0.0)));
                    k = K;
                }
                for (; k + 2 <= K; k += 2) {
                    const double v0 = m.xv[k], v1 = m.xv[k + 1];
                    const double sa = poly7(xm, v0), sb = poly7(xm, v1);
                    const double La = sa - s_hi, Lb = sb - sa;
                    s_hi = sb;
                    atomicMax(&mxc[k * MXCOLS], (unsigned long long)__double_as_longlong(fmax(fabs(La), 0.0)));
                    atomicMax(&mxc[(k + 1) * MXCOLS], (unsigned long long)__double_as_longlong(fmax(fabs(Lb), 0.0)));
                }
                for (; k < K; ++k) {
                    const double st = poly7(xm, m.xv[k]);
                    const double L = st - s_hi;
                    s_hi = st;
                    atomicMax(&mxc[k * MXCOLS], (unsigned long long)__double_as_longlong(fmax(fabs(L), 0.0)));
                }
                if constexpr (TRACE) u_end = last_crossing();
                if (PR ? (k0 + 1 < K) : (K > 1)) last_len = u_end * scale;                    // (only its NaN-ness is used)
                if (K > 0 && cnt && !(poly5(q.h, u_end) > Ck().z_hi)) my_flags |= 8;         // last sample of the ray
            }
            if (reduce && cnt && K > 0) my_flags |= (last_len != last_len) ? 1 : 2;
            if constexpr (TRACE) {
                // the lanes' flags as ONE wave-uniform word from here on (flush ORs the lanes' words: the same result), so that no lane
                // carries them through the march
                int wave_flags = 0;
#pragma unroll
                for (int b = 1; b <= 8; b <<= 1) if (__any(my_flags & b)) wave_flags |= b;
                my_flags = wave_flags;
                // ---- the march of march_kernel<T2, false, 1>, on the values a record would have carried
                {
                    asm volatile("" ::: "memory");             // (the parked polynomial is read back HERE, not forwarded past the folds in registers)
                    int tp = threadIdx.x;
                    asm volatile("" : "+v"(tp));
                    const double* const park = trace_park(m, cm.nz) + tp;
#pragma unroll
                    for (int n = 0; n < PN; ++n) q.lon[n] = park[n * BLOCK];
                }
                double acc_w = 0.0, acc_h = 0.0;
                const double u0r = active ? u_first : 0.0, u1r = active ? u_hi : 0.0;
                const EpochCubes<T2, 1> one{{cm.v}};
                const unsigned long long live = __builtin_amdgcn_ballot_w64(active && mine);
                const LevelRec* const lev = Pk().lev + (int64_t)__builtin_amdgcn_readfirstlane(sl) * (cm.nz + 1);
                const bool lane_safe = lane_nocheck(u0r, u1r, active, mine, q, xc, cm.ny, cm.nx);
                if (__all(lane_safe)) march_slice_levels<T2, 1, true>(cm, one, m, q, xc, lev, u0r, u1r, K, clamp_lo, clamp_hi, live, &acc_w, &acc_h);
                else march_slice_levels<T2, 1, false>(cm, one, m, q, xc, lev, u0r, u1r, K, clamp_lo, clamp_hi, live, &acc_w, &acc_h);
                acc_w *= scale; acc_h *= scale;
                // (the ray's place in the output derived afresh behind the loop - tile_ray, as march_kernel has it - not carried across it)
                int to = threadIdx.x;
                asm volatile("" : "+v"(to));
                int64_t io; bool there;
                tile_ray(Pk(), t, to, io, there);
                if (there && mine) { const auto& oa = Pk(); const int64_t o = (int64_t)sl * oa.n + io; oa.wet[o] = acc_w + poison; oa.hyd[o] = acc_h + poison; }
            }
        }
    }
    flush();
    if (skip_on()) {
        __syncthreads();
        if (threadIdx.x == 0 && m.K[3] > 0) atomicAdd(Pk().nslow + 1, m.K[3]);
    }
}

template <typename T2, bool SLOW, bool LCC = false, int OM = 0, bool PR = false>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(SLOW ? 1 : 4, SLOW ? 8 : 4))) void crossings_kernel(CubeView<T2> c, RayParams P, LccParams proj) {
    pass1_tiles<T2, SLOW, LCC, OM, PR, false>(c, P, proj);
}

// ---- the one-kernel route: fit and march a tile's slice rays in ONE kernel, on a partition that was probed and is then proven ----------
// Only one fact forces two passes over the rays: nParts[k] = ceil(max over the slice of the level's length / max_seg) + 1 needs every ray,
// but only through a maximum - and a maximum is monotone.  The host (trace_one_pass) runs crossings_kernel reduce-only over a small list of
// tiles (the border of the scene and a coarse lattice: RayParams::tile_list), level_table_kernel on what that found, and
// partition_check_kernel<false>, which notes the probed nParts and what fill_partition derives from the flags (OP_NPARTS, OP_BITS).  Then
// this kernel: pass 1's tile body as it stands - every ray folds into the real maxima and flags, seeded with the probed ones so that the
// wave bound skips nearly every level loop - and, from the registers the records would have been written from, pass 2's slice loop on the
// PROBED level records.  partition_check_kernel<true> recomputes nParts and the derived flags from the final maxima; when they equal the
// probed ones (integers and three bits: equality is a proof) the delays are, bit for bit, what the two passes give - same fit, same
// partition, same loop.  Anything else raises OP_NEED: a differing partition, a ray for the generic kernels, a non-finite ray.  The classic
// kernels are enqueued behind in every case, return at their top while OP_NEED is 0, and overwrite every output when it is not.
// GRID: march_kernel's (1: REGULAR, the only one built); OM: crossings_kernel's (1 or 2: a GRID batch).
template <typename T2, int GRID, int OM>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4, 4))) void trace_kernel(CubeView<T2> c, RayParams P, LccParams proj) {
    static_assert(GRID == 1 && sizeof(T2) == 8, "built for f32 cubes on exactly uniform axes");
    pass1_tiles<T2, false, false, OM, false, true>(c, P, proj);
}

// ---- pass 2: the parts march_kernel and march_epochs_kernel (epoch_kernels.h) share ---------------------------------
// What a slice's partition decides for every ray of the slice.
struct SlicePartition {
    double poison;          // NaN when the partition is undefined, else 0: added to every output of the slice
    bool clamp_lo, clamp_hi;
};

// nParts of level k of slice sl (delay.py:283) from the given partition or the slice's length maxima; diverged: the lengths ask for
// fewer than 2 or more than MAX_NPARTS parts (e.g. look vectors far from unit length) - the loops run with 2, the caller flags it.
// (RP: RayParams, by value or in the kernarg segment - RayKernArgs; so below)
template <typename RP>
__device__ __forceinline__ int level_nparts(const RP& P, int sl, int k, bool& diverged) {
    int np;
    if (P.nparts_override) np = P.nparts_override[(int64_t)sl * MAX_LEVELS + k];
    else {
        const double parts = ceil(__longlong_as_double((long long)P.maxlen_bits[(int64_t)sl * MAX_LEVELS + k]) / P.max_seg) + 1.0;   // delay.py:283
        np = (parts >= 1.0 && parts <= (double)MAX_NPARTS) ? (int)parts : -1;
    }
    diverged = np < 2 || np > MAX_NPARTS;
    return diverged ? 2 : np;
}
__device__ __forceinline__ double level_step(int np) { return 1.0 / ((double)np - 1.0); }       // np.linspace(0,1,np) (delay.py:287)
__device__ __forceinline__ double level_half_weight(double step) { return 0.5e-6 * step; }       // delay.py:314-315: end points get half of L*1e-6/(np-1)

// Integration partition of slice sl, after fill_levels (workgroup-uniform; called by every thread): the separate LDS arrays the
// per-ray-height loops and the generic kernel read, and what the partition decides for every ray of the slice.  (The light slice
// loop reads the same values from the level table: level_table_kernel.)
template <typename RP>
__device__ __forceinline__ SlicePartition fill_partition(const RP& P, const RaySmem& m, int sl, int K) {
    int tz = threadIdx.x;
    asm volatile("" : "+v"(tz));                   // (opaque: nothing derived from it is hoisted out of the tile loop and spilled)
    if (tz == 0) m.K[1] = 0;
    __syncthreads();
    for (int k = tz; k < K; k += BLOCK) {
        bool diverged;
        const int np = level_nparts(P, sl, k, diverged);
        if (diverged) {                       // refuse to loop over diverged lengths
            atomicOr(P.flags + sl, 16);       // RDR_FLAG_DIVERGED
            m.K[1] = 1;
        }
        m.np[k] = np;
        m.step[k] = level_step(np);
        m.hs[k] = level_half_weight(m.step[k]);
    }
    __syncthreads();
    const int flags_in = P.flags[sl];
    SlicePartition s;
    // Every output of the slice is NaN when its partition is undefined: diverged lengths, or a NaN ray length anywhere in
    // the slice - ndarray.max poisons nParts and the reference raises (delay.py:283).  The synchronous entry points raise
    // the same error; a caller of the asynchronous ones (device arrays, no host round trip) gets NaN, never a finite
    // delay computed with a partition the reference does not define.
    s.poison = (m.K[1] || (flags_in & (1 | 32))) ? qnan() : 0.0;      // (32: a per-ray height below the slice table's)
    s.clamp_lo = !(flags_in & 4);               // ALL first samples below zmin  (delay.py:306-307)
    s.clamp_hi = !(flags_in & 8);               // ALL last samples above zmax   (delay.py:310-311)
    return s;
}

// The record of level k of a slice (after fill_levels; np: the level's nParts): what the slice loop reads of it.
__device__ __forceinline__ LevelRec make_level_rec(const RaySmem& m, int nz, int k, int np) {
    const int kzk = m.kz[k], last = nz - 1;
    const int zb = max(window2_base(nz, kzk), 0);            // (nz = 2: the window is never trusted, only in-range reads matter)
    LevelRec r;
    r.step = level_step(np); r.hs = level_half_weight(r.step); r.xv = m.xv[k];
    r.zmid = m.ax.ez[min(zb + 1, last)].x; r.r0 = m.ax.ez[zb].y; r.r1 = m.ax.ez[min(zb + 1, last)].y;
    r.gk = m.ax.ez[kzk].x; r.rk = m.ax.ez[kzk].y;
    r.npkz = np | (kzk << 17); r.pad[0] = r.pad[1] = r.pad[2] = 0;
    return r;
}

// The level table of pass 2 (RayParams::lev): workgroup b writes the nz + 1 records of slice first_slice + b from what fill_partition
// reads - the slice's height, zref, the z axis and its partition (length maxima or given nParts), all on the device, no host round trip.
// A kernel of its own, once per pass 2: the march kernels read the table through the scalar cache, which does not see vector stores of the
// same kernel - the table is complete at a kernel boundary of the stream.  It only reads the partition: flags are fill_partition's.
// Launched with ray_smem_bytes(0, 0, nz, 1, 1) of LDS (the z table and the level arrays; no horizontal axis).
template <typename T2>
__global__ __launch_bounds__(BLOCK) void level_table_kernel(CubeView<T2> c, RayParams P, int first_slice, LevelRec* table) {
    if (P.one_pass != nullptr && P.one_pass[OP_NEED] == 0) return;                // (enqueued behind trace_kernel: pass1_tiles)
    c.exact_y = 1; c.exact_x = 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const RaySmem m = carve_smem(smem_raw, c.ny, c.nx, c.nz, 1, 1);
    fill_axes(c, m);
    const int sl = first_slice + (int)blockIdx.x;
    const int K = fill_levels(c.nz, m, P.hts ? P.hts[sl] : P.ht, P.zref);
    LevelRec* const out = table + (int64_t)sl * (c.nz + 1);
    for (int k = threadIdx.x; k <= c.nz; k += BLOCK) {
        LevelRec r;
        if (k < K) {
            bool diverged;
            r = make_level_rec(m, c.nz, k, level_nparts(P, sl, k, diverged));
        } else if (k == K && K > 0) {
            // one record past the last level (K <= nz-1): the "next level" of the last one repeats its top abscissa with weight 0,
            // so the loop computes du1 = X(v) - X(v) = 0 and adds 0 * 0 to the top weight instead of branching on `more`
            bool diverged;
            r = make_level_rec(m, c.nz, K - 1, level_nparts(P, sl, K - 1, diverged));
            r.hs = 0.0; r.npkz = 2 | (m.kz[K - 1] << 17);
        } else {
            r.xv = r.hs = r.step = r.zmid = r.r0 = r.r1 = r.gk = r.rk = 0.0;     // (the unconditional load of record 0 of a slice without levels)
            r.npkz = 0; r.pad[0] = r.pad[1] = r.pad[2] = 0;
        }
        out[k] = r;
    }
}

// The sines and cosines of a GRID batch's ny latitudes and nx longitudes for trace_kernel (RayParams::grid_trig): what tile_trig computes per
// tile in pass 1, by the same sincos on the same argument - the same bits.
__global__ __launch_bounds__(BLOCK) void grid_trig_kernel(RayParams P, double* trig) {
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < P.ny + P.nx; j += (int64_t)gridDim.x * BLOCK) {
        double sv, cv;
        sincos((j < P.ny ? P.ypts[j] : P.xpts[j - P.ny]) * DEG_TO_RAD, &sv, &cv);
        trig[2 * j] = sv; trig[2 * j + 1] = cv;
    }
}

// The one-kernel route's two looks at the partition of slice 0 (one workgroup; K levels): nParts[k] as level_table_kernel derives them and the
// three things fill_partition derives from the flags.  VERIFY false, after the probe: noted in P.one_pass, OP_NEED cleared.  VERIFY true, after
// trace_kernel has folded every ray: compared with the note - any difference raises OP_NEED - and RDR_FLAG_DIVERGED set as fill_partition sets
// it (the classic march behind, which would, may not run).
template <bool VERIFY>
__global__ __launch_bounds__(BLOCK) void partition_check_kernel(RayParams P, int K) {
    __shared__ int s_diverged, s_differs;
    if (threadIdx.x == 0) { s_diverged = 0; s_differs = 0; }
    __syncthreads();
    int* const op = P.one_pass;
    for (int k = threadIdx.x; k < K; k += BLOCK) {
        bool diverged;
        const int np = level_nparts(P, 0, k, diverged);
        if (diverged) s_diverged = 1;
        if (VERIFY) { if (op[OP_NPARTS + k] != np) s_differs = 1; }
        else op[OP_NPARTS + k] = np;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int f = P.flags[0];
        const int bits = ((s_diverged || (f & (1 | 32))) ? 1 : 0) | ((f & 4) ? 0 : 2) | ((f & 8) ? 0 : 4);      // poison, clamp_lo, clamp_hi
        if (VERIFY) {
            if (s_diverged) atomicOr(P.flags, 16);
            if (s_differs || bits != op[OP_BITS]) op[OP_NEED] = 1;
            if (op[OP_NEED] != 0) op[OP_REDO] += 1;
        } else { op[OP_BITS] = bits; op[OP_NEED] = 0; }
    }
}

// Thread tl of tile t (within its slice) -> ray i of the batch; active: the ray exists (false: tile padding).
template <typename RP>
__device__ __forceinline__ void tile_ray(const RP& P, int64_t t, int tl, int64_t& i, bool& active) {
    if (P.origin_mode == 0) {
        const int64_t ty = t / P.tiles_x, tx = t - ty * P.tiles_x;
        const int64_t row = ty * TILE + (tl >> 4), col = tx * TILE + (tl & 15);
        active = row < P.ny && col < P.nx;
        i = row * P.nx + col;
    } else {
        i = t * BLOCK + tl;
        active = i < P.n;
    }
}

// A light ray's record (w: the ray's slot of the workspace, ns: its field stride): the three ray polynomials and the crossing
// polynomial.  The level crossings come from the latter as the loop reaches them (7 FMAs, no global loads inside the loop besides
// the gathers, so the only memory waits are on a sample's own corners).
// A record is read once per pass 2 and there are 232 B of it per ray - 3.7 GB on the headline step, against a cube of 58 MB that every
// sample gathers from: the loads are marked nontemporal (record_field), so that the stream of records does not push the cube's lines
// out of the L2.  Same values, so same bits.
__device__ __forceinline__ double record_field(const double* w, int64_t ns, int f) { return __builtin_nontemporal_load(&w[(int64_t)f * ns]); }
__device__ __forceinline__ void load_ray_record(const double* w, int64_t ns, RayPoly& q, double (&xc)[PX]) {
#pragma unroll
    for (int n = 0; n < PN; ++n) {
        q.h[n] = record_field(w, ns, WS_POLY_H + n);
        q.lat[n] = record_field(w, ns, WS_POLY_LAT + n);
        q.lon[n] = record_field(w, ns, WS_POLY_LON + n);
    }
#pragma unroll
    for (int n = 0; n < PX; ++n) xc[n] = record_field(w, ns, WS_XPOLY + n);
}

// The no-check proof of a lane (REGULAR grids; the kernels take it wave-wide: __all); u0r, u1r: fields WS_U0, WS_U1 of its record,
// passed by value (loaded inside, the per-ray-height instantiations allocate registers differently: profiles/r15_march_fold_regs.txt).
// Bounds of the horizontal cell search, decided ONCE per wave from the polynomial coefficients.  Every sample's ray parameter lies between the ray's crossings: the two of the
// first level (u0, u1 of the record) and X(v_k), |v_k| <= 1, whose magnitude is at most sum |x_k|.  So when |u0|, |u1| and
// sum |x_k| are all <= 1.001 (the crossings sit inside the fit range [-1, 1] by construction; diverged or non-finite rays fail this),
// every sample has |u| <= 1.001 and p(u) lies within c0 +- 1.006 sum_{k>=1} |c_k| (1.001^5 < 1.006).  When that interval is inside
// [0, n-1) for the index-space lat AND lon polynomials of every ray of the wave, no gather can leave the cube and the per-sample
// bounds tests (4 compares + the rare-path plumbing) are compiled out of the loop.  Lanes of tile padding get a harmless in-range
// polynomial (written into q / xc here); a wave holding a generic ray (whose record is not a polynomial), a diverged ray or a ray
// near the cube's edge keeps the checked loop.
__device__ __forceinline__ bool lane_nocheck(double u0r, double u1r, bool active, bool mine, RayPoly& q, double (&xc)[PX], int ny, int nx) {
    if (!active) {
#pragma unroll
        for (int n = 0; n < PN; ++n) { q.lat[n] = 0.0; q.lon[n] = 0.0; }
        q.lat[0] = 0.5; q.lon[0] = 0.5;
#pragma unroll
        for (int n = 0; n < PX; ++n) xc[n] = 0.0;
        u0r = 0.0; u1r = 0.0;
    }
    auto inside = [&](const double* cf, int n) {
        const double r = 1.006 * (fabs(cf[1]) + fabs(cf[2]) + fabs(cf[3]) + fabs(cf[4]) + fabs(cf[5]));
        return (cf[0] - r >= 0.0) & (cf[0] + r < (double)(n - 1));
    };
    double xs = 0.0;
#pragma unroll
    for (int n = 0; n < PX; ++n) xs += fabs(xc[n]);
    return (mine || !active) && (fabs(u0r) <= 1.001) && (fabs(u1r) <= 1.001) && (xs <= 1.001) && inside(q.lat, ny) && inside(q.lon, nx);
}

// ---- pass 2: the two level loops of the light rays, for E cubes on one ray geometry ----------------------------------
// march_kernel runs them with E = 1 on its own cube, march_epochs_kernel (epoch_kernels.h) with the E epochs of a stacked launch: per
// sample the ray polynomials, the cell searches, the z window and the corner offset run once, then E corner-pair gathers (independent of
// each other) and E (wet, hydro) accumulators.  Per epoch the instructions and their operands do not depend on E, which is why epoch e of
// a series is bit for bit the one-cube call on cube e.
// Every distinct sample point of the ray once, level by level.  The sample schedule (level k, fraction j/(np-1)) is the same for every
// ray of the slice, so the loop counters live in scalar registers.  A sample shared by two segments (top of k = bottom of k+1,
// losreader.py:811-812) is evaluated once and carries both trapezoid end weights; a level is its interior samples (usually none or one)
// plus its top sample.  Latency is hidden by the waves per SIMD (and the E gathers), not by batching samples inside a lane.

// A level's top sample or the ray's first sample (sample_issue MODE 1) at ray parameter us.
template <typename T2, int E, bool NC>
__device__ __forceinline__ void issue_top(const CubeView<T2>& c, const EpochCubes<T2, E>& ev, const RaySmem& m, const RayPoly& q, double us, int zbase,
                                          bool floor_it, bool ceil_it, PendingSample<T2, E>& s) {
    double ph = poly5(q.h, us);
    const double plat = poly5(q.lat, us), plon = poly5(q.lon, us);       // delay.py:295 through the ray polynomials
    // all-pixels z-clamp of the very first / very last sample (delay.py:306-311): when it applies every pixel is
    // below (above) the cube, so "set to zmin" == max(ph, zmin).  Slice-uniform conditions: real (scalar) branches,
    // so the two samples of a ray they can apply to are the only ones that pay for them.
    if (floor_it) { asm volatile("" ::: "memory"); ph = fmax(ph, c.z_lo); }
    if (ceil_it) { asm volatile("" ::: "memory"); ph = fmin(ph, c.z_hi); }
    sample_issue<T2, 1, NC, E>(c, ev, m.ax, plat, plon, ph, zbase, s);   // delay.py:298,319
}

// The E values of a sample set into the E accumulator pairs with trapezoid weight wv.  (The epoch index is a template argument, not a
// loop counter: the sample set is split into registers before any loop is unrolled, which the E = 1 instantiations need to come out
// as march_kernel's hand-written loops did - profiles/r16_loop_fold_regs.txt.)
template <typename T2, int E, int e = 0>
__device__ __forceinline__ void finish_into(const PendingSample<T2, E>& s, double wv, double* acc_w, double* acc_h) {
    double vw, vh;
    sample_finish_lerp(s, vw, vh, e);
    acc_w[e] = fma(wv, vw, acc_w[e]); acc_h[e] = fma(wv, vh, acc_h[e]);          // delay.py:323
    if constexpr (e + 1 < E) finish_into<T2, E, e + 1>(s, wv, acc_w, acc_h);
}

// The slice loop: every ray of the slice starts at the slice's height.  u0, u1: fields WS_U0, WS_U1 of the ray's record (the crossings
// of its first level); live: the lanes whose samples count - a lane of tile padding or a generic ray (its record is not a polynomial)
// computes garbage that is never stored, and must not decide a wave-uniform branch.  Adds into acc_w[E], acc_h[E] (per unit of u).
// A level record in scalar registers: the fields the slice loop reads, loaded through the constant address space (scalar loads).
struct LevelRegs { double xv, hs, step, zmid, r0, r1, gk, rk; int npkz; };
typedef __attribute__((address_space(4))) const LevelRec ConstLevelRec;
__device__ __forceinline__ LevelRegs load_level(const ConstLevelRec* r) {
    LevelRegs v;
    v.xv = r->xv; v.hs = r->hs; v.step = r->step; v.zmid = r->zmid; v.r0 = r->r0; v.r1 = r->r1; v.gk = r->gk; v.rk = r->rk; v.npkz = r->npkz;
    return v;
}

// lev: the slice's records in the level table (wave-uniform pointer; K + 1 of them are read).
template <typename T2, int E, bool NC>
__device__ __forceinline__ void march_slice_levels(const CubeView<T2>& c, const EpochCubes<T2, E>& ev, const RaySmem& m, const RayPoly& q, const double (&xc)[PX],
                                                   const LevelRec* lev, double u0, double u1, int K, bool clamp_lo, bool clamp_hi, unsigned long long live,
                                                   double* acc_w, double* acc_h) {
    // Everything slice-uniform about a level sits in scalar registers, loaded ONE LEVEL AHEAD: `cur` is the level being integrated, `nxt`
    // is requested at its top and first needed behind its top sample's gathers (loaded at the point of use, the scalar-cache latency
    // would stand where the LDS latency stood).  Record 0 of a slice without levels is zeros (level_table_kernel).
    const ConstLevelRec* rec = (const ConstLevelRec*)(size_t)lev;
    LevelRegs cur = load_level(rec);
    int np = cur.npkz & 0x1ffff, kz = cur.npkz >> 17;                        // np >= 2 (level_nparts)
    double hs = cur.hs;
    double u_k = u0;
    double u_last = u1;
    double du = u_last - u_k;
    // the ray's very first sample is the BOTTOM of its segment: when that is a model node (origin at or below it), the
    // two-entry z window must start one interval lower
    if (K > 0) {
        PendingSample<T2, E> s;
        issue_top<T2, E, NC>(c, ev, m, q, fma(0.0 * cur.step, du, u_k), window2_base(c.nz, kz - ((m.lo[0] <= m.ax.ez[kz].x) ? 1 : 0)), clamp_lo, false, s);
        finish_into(s, hs * fabs(du), acc_w, acc_h);
    }
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const LevelRegs nxt = load_level(rec + k + 1);                       // (the record after the last level: the sentinel)
        const int zbase = window2_base(c.nz, kz);                            // first table entry of the two-entry z window
        const bool more = k + 1 < K;
        // trapezoid weights per unit of u (delay.py:314-315): interior samples, and the top one with both its segments.  The weight is the
        // segment's LENGTH (a norm, losreader.py:821): |du| - an origin above zref in zref's model interval walks its one segment downwards
        const double w_mid = (2.0 * hs) * fabs(du);
        if (np > 2) {
            const double step = cur.step, gk = cur.gk, rk = cur.rk;
#pragma unroll 1
            for (int j = 1; j < np - 1; ++j) {                               // low + frac * (high - low), delay.py:292
                PendingSample<T2, E> s;
                const double us = fma((double)j * step, du, u_k);
                const double ph = poly5(q.h, us), plat = poly5(q.lat, us), plon = poly5(q.lon, us);
                int iz = kz;                                                 // strictly inside model interval kz: one table entry, no select
                s.tz = (ph - gk) * rk;
                if (!(s.tz >= 0.0) || !(s.tz <= 1.0)) cell_exact(m.ax.ez, c.nz, ph, iz, s.tz);   // rare
                gather_corners<T2, E, true, NC>(c, ev, m.ax, plat, plon, iz, s);
                finish_into(s, w_mid, acc_w, acc_h);
            }
        }
        // top sample: its gathers are issued first, the next level's crossing (7 FMAs that need no memory) is computed
        // while they are in flight, then the sample is finished with the weight of both its segments
        PendingSample<T2, E> top;
        {
            const double us = u_k + du;                                      // fraction exactly 1.0, as np.linspace returns it
            double ph = poly5(q.h, us);
            const double plat = poly5(q.lat, us), plon = poly5(q.lon, us);   // delay.py:295 through the ray polynomials
            if (clamp_hi && !more) { asm volatile("" ::: "memory"); ph = fmin(ph, c.z_hi); }      // delay.py:310-311 (slice-uniform branch)
            // z cell: the top sits on node g[zbase+1] within the residual of the three-iteration crossing - ABOVE it for every ray
            // whose zenith angle falls with height (profiles/r06_nodetop_ab.txt).  When no live lane of the wave is below the node
            // (one compare + a scalar test) the cell index is the scalar zbase+1 and the weight one multiplication; otherwise the
            // per-lane two-entry window.  Same values either way.
            const double d = ph - cur.zmid;
            int iz; bool ok;
            if (__builtin_expect((__builtin_amdgcn_ballot_w64(!(d >= 0.0)) & live) == 0ULL, 1)) {
                iz = zbase + 1;
                top.tz = d * cur.r1;
                ok = top.tz <= 1.0;                                                                // (idle lanes: NaN)
            } else {
                double ds = d;
                asm volatile("" : "+v"(ds));                                                       // (nothing of this block is hoisted into the fast path)
                const bool up = ds >= 0.0;
                iz = zbase + (int)up;
                top.tz = fma(ds, up ? cur.r1 : cur.r0, up ? 0.0 : 1.0);
                ok = (top.tz >= 0.0) & (top.tz <= 1.0);
            }
            if (!(ok & (c.nz >= 4))) cell_exact(m.ax.ez, c.nz, ph, iz, top.tz);                  // rare
            gather_corners<T2, E, true, NC>(c, ev, m.ax, plat, plon, iz, top);                   // delay.py:298,319
        }
        // (the record after the last level: same abscissa, weight 0 - see level_table_kernel)
        const double t2 = poly7(xc, nxt.xv);
        const double du1 = t2 - u_last, hs1 = nxt.hs;
        u_last = t2;
        const double w_top = fma(hs1, fabs(du1), hs * fabs(du));
        finish_into(top, w_top, acc_w, acc_h);
        u_k += du; du = du1; hs = hs1;
        np = nxt.npkz & 0x1ffff; kz = nxt.npkz >> 17;
        cur = nxt;
    }
}

// The per-ray-height loop (P.ht_ray): the level schedule (k, j) stays slice-uniform - scalar loop counters, the partition
// of the slice - and a lane joins it at its own first level k0 (first_level; K: none) with its own first sample; until then it idles
// (execution mask).  The loop starts at the wave's lowest k0.  Same arithmetic per sample as the slice loop, so that equal heights give
// the slice kernel's delays bit for bit.  lo_first: the bottom of the lane's first level.
// (K by reference, as the kernels' own loops read it: by value the compiler allocates the registers of the REGULAR f32 instantiation
// differently - 16 B of scratch instead of 24 - and this is a fold, not a tuning: profiles/r16_loop_fold_regs.txt.)
template <typename T2, int E, bool NC>
__device__ __forceinline__ void march_ray_height_levels(const CubeView<T2>& c, const EpochCubes<T2, E>& ev, const RaySmem& m, const RayPoly& q, const double (&xc)[PX],
                                                        double u0, double u1, const int& K, int k0, double lo_first, bool clamp_lo, bool clamp_hi,
                                                        double* acc_w, double* acc_h) {
    int kmin = k0;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) kmin = min(kmin, __shfl_xor(kmin, off, 64));
    kmin = __builtin_amdgcn_readfirstlane(kmin);
    // every lane's FIRST sample (the bottom of its own first level) in one evaluation for the whole wave - per-lane level
    // constants from LDS - instead of once per distinct k0 inside the loop (a DEM tile has a dozen of those)
    const bool has = k0 < K;
    const int kf = has ? k0 : 0;
    double u_k = has ? u0 : 0.0, u_last = has ? u1 : 0.0;
    double du = u_last - u_k;
    if (K > 0) {
        const int kzf = m.kz[kf];
        PendingSample<T2, E> s;
        issue_top<T2, E, NC>(c, ev, m, q, fma(0.0 * m.step[kf], du, u_k), window2_base(c.nz, kzf - ((lo_first <= m.ax.ez[kzf].x) ? 1 : 0)), clamp_lo, false, s);
        if (has) finish_into(s, m.hs[kf] * fabs(du), acc_w, acc_h);
    }
#pragma unroll 1
    for (int k = kmin; k < K; ++k) {
        const int np = __builtin_amdgcn_readfirstlane(m.np[k]);
        const int kz = __builtin_amdgcn_readfirstlane(m.kz[k]);
        const double step = m.step[k], hs = m.hs[k];
        const bool more = k + 1 < K;
        if (k >= k0) {
            const int zbase = window2_base(c.nz, kz);
            const double w_mid = (2.0 * hs) * fabs(du);
#pragma unroll 1
            for (int j = 1; j < np - 1; ++j) {          // strictly inside model interval kz (sample_issue MODE 2)
                PendingSample<T2, E> s;
                const double us = fma((double)j * step, du, u_k);
                const double ph = poly5(q.h, us);
                const double plat = poly5(q.lat, us), plon = poly5(q.lon, us);
                sample_issue<T2, 2, NC, E>(c, ev, m.ax, plat, plon, ph, kz, s);
                finish_into(s, w_mid, acc_w, acc_h);
            }
            PendingSample<T2, E> top;
            issue_top<T2, E, NC>(c, ev, m, q, u_k + du, zbase, false, clamp_hi && !more, top);
            double du1 = 0.0;
            double w_top = hs * fabs(du);
            if (more) {
                const double t2 = poly7(xc, m.xv[k + 1]);
                du1 = t2 - u_last; u_last = t2;
                w_top = fma(m.hs[k + 1], fabs(du1), w_top);
            }
            finish_into(top, w_top, acc_w, acc_h);
            u_k += du; du = du1;
        }
    }
}

// ---- pass 2: trapezoid integration of both fields along every ray (delay.py:285-323) -------------------------------
// SLOW as in crossings_kernel: <false> integrates the classified-fast rays with the light geodesy, <true> the rest
// with the generic one (and returns immediately when there are none).
// GRID (light kernel only), known at compile time so that the per-sample code carries no trace of the other variants:
//   1 (REGULAR): both horizontal axes are exactly uniform and the cube allows 32-bit offsets - the usual lat/lon or LCC model grid;
//   2 (TABLES): both axes only NEARLY uniform (e.g. 0.1-degree nodes stored as float32) - guess-and-verify against the LDS tables -
//               and 32-bit offsets;   0: whatever the run-time flags say.
// PR (light kernel only): per-ray origin heights (P.ht_ray) - its own instantiation, the slice kernels carry none of it.
template <typename T2, bool SLOW, int GRID = 0, bool PR = false>
// (f64 cubes - azimuth-time-grid blends - hold 8 x 16 B of corners per sample: three waves per SIMD without scratch beat four with 80 B of
// it, 6.8 against 11.4 ms per 16 M rays; the per-ray-height instantiation, 24 B of scratch at four waves, is better off as it is: 5.7 against 6.4 ms)
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(SLOW ? 1 : (sizeof(T2) == 16 ? 3 : 4), SLOW ? 8 : (sizeof(T2) == 16 ? 3 : 4)))) void march_kernel(CubeView<T2> c_in, RayParams P, LccParams proj) {
    static_assert(!SLOW || !PR, "the generic kernel looks at P.ht_ray at run time");
    if (P.one_pass != nullptr && P.one_pass[OP_NEED] == 0) return;                // (enqueued behind trace_kernel: pass1_tiles)
    if (SLOW && *P.nslow == 0) return;
    const bool per_ray = PR || (SLOW && P.ht_ray != nullptr);
    // (the uniform parameters of the tile body: crossings_kernel.  The cube view stays by value: the level loops read it as SGPR operands)
    auto Pk = [&]() -> decltype(auto) { if constexpr (SLOW) return (P); else return (ray_args<T2>()->P); };
    constexpr bool REGULAR = GRID == 1;
    CubeView<T2> c = c_in;
    if (REGULAR) { c.exact_y = 1; c.exact_x = 1; c.small = 1; }
    if (GRID == 2) { c.exact_y = 0; c.exact_x = 0; c.uni_y = 1; c.uni_x = 1; c.small = 1; }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const RaySmem m = carve_smem(smem_raw, c.ny, c.nx, c.nz, c.exact_y, c.exact_x);
    // f64 cubes on exactly uniform axes (round 4): a wave's footprint of one model level - 4 x 4 cube columns x 3 z entries of 16 B -
    // staged in LDS, the eight corners of every sample of the level read from there (STAGED below)
    constexpr bool STAGED = !SLOW && !PR && REGULAR && sizeof(T2) == 16;
    constexpr int STAGE_N = 48;                        // [z 0..2][y 0..3][x 0..3]
    __shared__ T2 s_stage[STAGED ? (BLOCK / 64) * STAGE_N : 1];
    fill_axes(c, m);
    const int tid = threadIdx.x;
    int K = 0, slice = -1;
    double poison = 0.0;
    bool clamp_lo = false, clamp_hi = false, clamp_any = false;
    TileWalk walk(P.tile_count, P.tile_ctr, m.K + 2);
    int64_t lt;
    while (walk.next(Pk().tile_count, lt)) {
        const auto& pa = Pk();                             // (this site: the tile's place in the batch, its rays and their records)
        const int64_t tg = pa.tile_begin + lt;             // tile of the batch; t: tile within its slice
        const int sl = (int)(tg / pa.tiles_per_slice);
        const int64_t t = tg - (int64_t)sl * pa.tiles_per_slice;
        if (sl != slice) {                                 // (workgroup-uniform) the slice's level table and integration partition
            slice = sl;
            K = fill_levels(c.nz, m, pa.hts ? pa.hts[sl] : pa.ht, pa.zref);
            const SlicePartition part = fill_partition(pa, m, sl, K);
            poison = part.poison; clamp_lo = part.clamp_lo; clamp_hi = part.clamp_hi;
            clamp_any = clamp_lo | clamp_hi;
        }
        int tl = threadIdx.x;
        asm volatile("" : "+v"(tl));                       // per-tile opaque copy of the thread index (see crossings_kernel)
        int64_t i; bool active;
        tile_ray(pa, t, tl, i, active);
        const double* w = pa.ws + (lt * BLOCK + tl);
        const int64_t ns = pa.nslots;
        const double scale_rec = SLOW ? w[(int64_t)WS_SCALE * ns] : record_field(w, ns, WS_SCALE);   // light ray: ray length per unit of u (> 0 or NaN); generic ray: 0
        const bool fast_ok = !active || scale_rec != 0.0;
        const bool mine = SLOW ? !fast_ok : fast_ok;
        if (SLOW && !__any(mine)) continue;
        double acc_w = 0.0, acc_h = 0.0;
        // per-ray heights: the ray's first level of the slice table, found exactly as pass 1 found it (idle lanes: none)
        int k0 = 0; double lo_first = K > 0 ? m.lo[0] : 0.0;
        if (PR || SLOW) {
            if (per_ray) k0 = (active && mine) ? first_level(m.ax.ez, c.nz, m.lo, m.hi, m.kz, K, pa.ht_ray[i], lo_first) : K;
        }
        if constexpr (!SLOW) {
            // ---- light rays: the two level loops above, on this one cube ------------------------------------------------
            RayPoly q;
            double xc[PX];
            load_ray_record(w, ns, q, xc);
            const double scale = scale_rec;
            const double u0r = record_field(w, ns, WS_U0), u1r = record_field(w, ns, WS_U1);
            const EpochCubes<T2, 1> one{{c.v}};
            const unsigned long long live = __builtin_amdgcn_ballot_w64(active && mine);
            // the slice's records of the level table (per tile, from the scalar slice index: a pointer kept across the slice test would
            // not be wave-uniform for the compiler, and the records would come through vector loads)
            const LevelRec* const lev = PR ? nullptr : pa.lev + (int64_t)__builtin_amdgcn_readfirstlane(sl) * (c.nz + 1);
            auto run = [&](auto nochk) {
                constexpr bool NC = decltype(nochk)::value;
                if constexpr (PR) march_ray_height_levels<T2, 1, NC>(c, one, m, q, xc, u0r, u1r, K, k0, lo_first, clamp_lo, clamp_hi, &acc_w, &acc_h);
                else march_slice_levels<T2, 1, NC>(c, one, m, q, xc, lev, u0r, u1r, K, clamp_lo, clamp_hi, live, &acc_w, &acc_h);
            };
            // the wave-wide no-check proof (lane_nocheck): bounds of the cell search from the polynomial coefficients
            bool lane_safe = false;
            if (REGULAR) lane_safe = lane_nocheck(u0r, u1r, active, mine, q, xc, c.ny, c.nx);
            // ---- f64 cubes: the level's footprint through LDS --------------------------------------------------------------------
            // An f64 cube doubles the bytes of every gather (4 x 32 B per lane and sample): the instantiation is bound by the vector L1's
            // 64 B/clk return path, not by instruction issue (6.8 against 5.0 ms per 16 M rays, round 3).  But the 64 rays of a wave
            // (4 x 16 neighbouring pixels) sit in one or two cube cells at any given level: per level the wave loads the 4 x 4 columns
            // around lane 0's cell, z entries zb .. zb+2 (48 lanes, ONE 16 B load each), into LDS and every sample of the level reads
            // its eight corners from there (128 B/clk, broadcast) - same operands, same arithmetic: the same bits.  A sample whose
            // cell leaves the staged block for ANY lane of the wave (coarse scenes, large look-angle gradients) takes the direct
            // gathers, wave-uniformly.  Only for waves with the no-check proof above (cells inside the cube by construction).
            auto run_staged = [&]() {
                T2* const st = s_stage + (tl >> 6) * STAGE_N;
                const int lane = tl & 63;
                unsigned lane_off = ((unsigned)((lane >> 2) & 3) * (unsigned)c.nx + (unsigned)(lane & 3)) * (unsigned)c.nz + (unsigned)(lane >> 4);
                asm volatile("" : "+v"(lane_off));        // (opaque: the block's base below stays ONE scalar product, not two vector multiplies per level)
                const bool loader = lane < STAGE_N;
                bool stage_on = true;                     // wave-uniform: off for the rest of the tile once a level's cells leave the block
                                                          // (the footprint is set by scene spacing / cube spacing: a coarse scene never fits)
                const char* const vb = reinterpret_cast<const char*>(c.v);
                const size_t rowx = (size_t)c.nz * sizeof(T2), rowy = (size_t)c.nx * rowx;
                int fy0 = 0, fx0 = 0, zb = 0;
                // the eight corners of the sample in cell (iy, ix, iz): from the staged block when every lane's cell is in it
                auto fetch = [&](int iy, int ix, int iz, PendingSample<T2>& sm) {
                    const unsigned ry = (unsigned)(iy - fy0), rx = (unsigned)(ix - fx0), rz = (unsigned)(iz - zb);
                    bool staged_here = false;
                    if (stage_on) {
                        const bool out = active & (max(max(ry, rx), rz + 1u) > 2u);
                        staged_here = __builtin_amdgcn_ballot_w64(out) == 0;
                        stage_on = staged_here;
                    }
                    if (staged_here) {
                        // (an LDS-address-space pointer, and a fence: left as a generic pointer the two branches' loads are merged into
                        // ONE set of flat loads behind a pointer select - LDS data through the flat path, slower than the gathers)
                        typedef decltype(T2().x) S1;
                        typedef S1 S2 __attribute__((ext_vector_type(2)));
                        typedef __attribute__((address_space(3))) S2 LdsS2;
                        const LdsS2* p = (const LdsS2*)st + (active ? (rz * 16u + ry * 4u + rx) : 0u);
                        auto get = [&](int i_, int o_) { const S2 t_ = p[o_]; sm.v[0][i_].x = t_.x; sm.v[0][i_].y = t_.y; };
                        get(0, 0); get(1, 16); get(2, 1); get(3, 17); get(4, 4); get(5, 20); get(6, 5); get(7, 21);
                        asm volatile("" ::: "memory");
                    } else {
                        const unsigned off = (__umul24(__umul24((unsigned)iy, (unsigned)c.nx) + (unsigned)ix, (unsigned)c.nz) + (unsigned)iz) * (unsigned)sizeof(T2);
                        const T2* p00 = reinterpret_cast<const T2*>(vb + off);
                        const T2* p01 = reinterpret_cast<const T2*>(vb + rowx + off);
                        const T2* p10 = reinterpret_cast<const T2*>(vb + rowy + off);
                        const T2* p11 = reinterpret_cast<const T2*>(vb + rowy + rowx + off);
                        T2* const v = sm.v[0];
                        v[0] = p00[0]; v[1] = p00[1]; v[2] = p01[0]; v[3] = p01[1];
                        v[4] = p10[0]; v[5] = p10[1]; v[6] = p11[0]; v[7] = p11[1];
                    }
                };
                auto finish = [&](const PendingSample<T2>& sm, double wv) {
                    double vw, vh;
                    sample_finish_lerp(sm, vw, vh);
                    acc_w = fma(wv, vw, acc_w); acc_h = fma(wv, vh, acc_h);
                };
                int np = __builtin_amdgcn_readfirstlane(m.np[0]);
                int kz = __builtin_amdgcn_readfirstlane(m.kz[0]);
                double step = m.step[0], hs = m.hs[0];
                double u_k = w[(int64_t)WS_U0 * ns];
                double u_last = w[(int64_t)WS_U1 * ns];
                double du = u_last - u_k;
                if (K > 0) {                              // the ray's very first sample: direct gathers (its z window may start one interval lower)
                    PendingSample<T2> s0;
                    double ph = poly5(q.h, fma(0.0 * step, du, u_k));
                    const double plat = poly5(q.lat, fma(0.0 * step, du, u_k)), plon = poly5(q.lon, fma(0.0 * step, du, u_k));
                    if (clamp_lo) { asm volatile("" ::: "memory"); ph = fmax(ph, c.z_lo); }
                    sample_issue<T2, 1, true>(c, m.ax, plat, plon, ph, window2_base(c.nz, kz - ((m.lo[0] <= m.ax.ez[kz].x) ? 1 : 0)), s0);
                    finish(s0, hs * fabs(du));
                }
#pragma unroll 1
                for (int k = 0; k < K; ++k) {
                    zb = window2_base(c.nz, kz);
                    const bool more = k + 1 < K;
                    const double w_mid = (2.0 * hs) * fabs(du);
                    // the level's TOP sample first: its cell places the staged block
                    PendingSample<T2> top;
                    double ph = poly5(q.h, u_k + du);
                    const double plat = poly5(q.lat, u_k + du), plon = poly5(q.lon, u_k + du);
                    if (clamp_hi && !more) { asm volatile("" ::: "memory"); ph = fmin(ph, c.z_hi); }
                    int iy, ix, iz;
                    cell_xy<true, true>(m.ax.ey, c.ny, plat, c.y_lo, c.y_hi, c.inv_dy, true, true, iy, top.ty);
                    cell_xy<true, true>(m.ax.ex, c.nx, plon, c.x_lo, c.x_hi, c.inv_dx, true, true, ix, top.tx);
                    window2_cell(m.ax.ez, c.nz, ph, zb, c.nz >= 4, iz, top.tz);
                    if (stage_on) {
                        fy0 = min(max(__builtin_amdgcn_readfirstlane(iy) - 1, 0), c.ny - 4);
                        fx0 = min(max(__builtin_amdgcn_readfirstlane(ix) - 1, 0), c.nx - 4);
                        const unsigned base = (unsigned)__builtin_amdgcn_readfirstlane((fy0 * c.nx + fx0) * c.nz + zb);
                        __builtin_amdgcn_wave_barrier();          // (the previous level's readers are done: same wave, program order)
                        if (loader) st[lane] = c.v[base + lane_off];
                        __builtin_amdgcn_wave_barrier();
                    }
#pragma unroll 1
                    for (int j = 1; j < np - 1; ++j) {
                        PendingSample<T2> sm;
                        const double us = fma((double)j * step, du, u_k);
                        const double mh = poly5(q.h, us), mlat = poly5(q.lat, us), mlon = poly5(q.lon, us);
                        int my, mx, mz = kz;
                        cell_xy<true, true>(m.ax.ey, c.ny, mlat, c.y_lo, c.y_hi, c.inv_dy, true, true, my, sm.ty);
                        cell_xy<true, true>(m.ax.ex, c.nx, mlon, c.x_lo, c.x_hi, c.inv_dx, true, true, mx, sm.tx);
                        const double2 e0 = m.ax.ez[kz];
                        sm.tz = (mh - e0.x) * e0.y;
                        if (!(sm.tz >= 0.0) || !(sm.tz <= 1.0)) cell_exact(m.ax.ez, c.nz, mh, mz, sm.tz);   // rare
                        fetch(my, mx, mz, sm);
                        finish(sm, w_mid);
                    }
                    fetch(iy, ix, iz, top);
                    double du1 = 0.0, hs1 = 0.0;
                    double w_top = hs * fabs(du);
                    if (more) {
                        const double t2 = poly7(xc, m.xv[k + 1]);
                        du1 = t2 - u_last; u_last = t2; hs1 = m.hs[k + 1];
                        w_top = fma(hs1, fabs(du1), w_top);
                    }
                    finish(top, w_top);
                    u_k += du; du = du1; hs = hs1;
                    if (more) {
                        np = __builtin_amdgcn_readfirstlane(m.np[k + 1]);
                        kz = __builtin_amdgcn_readfirstlane(m.kz[k + 1]);
                        step = m.step[k + 1];
                    }
                }
            };
            if (REGULAR && __all(lane_safe)) {
                if constexpr (STAGED) {
                    if (Pk().stage_f64 && c.ny >= 4 && c.nx >= 4 && c.nz >= 3) run_staged();      // (the staged block holds z entries zb .. zb+2, zb >= 0)
                    else run(std::integral_constant<bool, true>{});
                } else run(std::integral_constant<bool, true>{});
            }
            else run(std::integral_constant<bool, false>{});
            acc_w *= scale; acc_h *= scale;
        } else {
            double vw_top = 0.0, vh_top = 0.0;    // sample values at the top of the previous segment (= bottom of this one)
            // generic rays: origin / look vector / origin frame; light rays: the three polynomials
            const double ox = w[(int64_t)(WS_ORIGIN + 0) * ns], oy = w[(int64_t)(WS_ORIGIN + 1) * ns], oz = w[(int64_t)(WS_ORIGIN + 2) * ns];
            const double lx = w[(int64_t)(WS_LOS + 0) * ns], ly = w[(int64_t)(WS_LOS + 1) * ns], lz = w[(int64_t)(WS_LOS + 2) * ns];
            const double nl2 = fma(lx, lx, fma(ly, ly, lz * lz));
            const double scale = nl2 * rsq_nr<2>(nl2);                  // |l|: ray length per unit of t
            // level crossings: streamed from the ray's side-buffer column one level ahead of their use, or - when pass 1 found the
            // side buffer full - recomputed with the very same iteration (same inputs, same instruction sequence)
            const int64_t sidx = mine ? (int64_t)w[(int64_t)WS_SIDE * ns] : -1;
            const double* const sd = (sidx >= 0 && P.side) ? P.side + sidx : nullptr;
            double t_hi = 0.0, t_next = 0.0, inv_cosf = 1.0;
            if (sd) { t_hi = sd[0]; if (k0 < K) t_next = sd[(int64_t)(k0 + 1) * P.side_cap]; }
            else if (mine && k0 < K) t_hi = toa_newton_t(ox, oy, oz, lx, ly, lz, lo_first, 10, 1.0);
    #pragma unroll 1
            for (int k = 0; k < K; ++k) {
                if (k < k0) continue;                // (per-ray heights: the ray joins the slice's level table at k0; else k0 = 0)
                const double t_lo = t_hi;
                if (sd) {
                    t_hi = t_next;
                    if (k + 2 <= K) t_next = sd[(int64_t)(k + 2) * P.side_cap];
                } else if (mine) {
                    t_hi = toa_newton_t(ox, oy, oz, lx, ly, lz, m.hi[k], k == k0 ? 10 : 3, inv_cosf);
                    if (k == k0) inv_cosf = (fabs(t_hi - t_lo) * scale) / (m.hi[k0] - lo_first);   // losreader.py:824-825, as in pass 1
                }
                const double dt = t_hi - t_lo;
                const int np = m.np[k];
                const double step = m.step[k];
                const double segw = (fabs(dt) * scale * 1.0e-6) * step;    // delay.py:315: L*1e-6/(np-1), L = |high-low| (losreader.py:821)
                const double dts = dt * step;                        // sample spacing: low + (j*step)*(high-low), delay.py:292
                const int kz = m.kz[k];
                // j = 0 of this segment is the SAME point as j = np-1 of the previous one (low_xyz is high_xyz,
                // losreader.py:811-812): its interpolated value is reused instead of recomputed (the reference evaluates
                // it twice and gets the same number both times).  The order of accumulation is unchanged.
                if (k > k0) { acc_w = fma(0.5 * segw, vw_top, acc_w); acc_h = fma(0.5 * segw, vh_top, acc_h); }
    #pragma unroll 1
                for (int j = (k == k0 ? 0 : 1); j < np; ++j) {
                    const double ts = fma((double)j, dts, t_lo);
                    double plon, plat, ph;
                    ecef2lla(fma(ts, lx, ox), fma(ts, ly, oy), fma(ts, lz, oz), plon, plat, ph);                     // delay.py:295
                    if (proj.kind == 1) { double px_, py_; lcc_forward(proj, plat, plon, px_, py_); plon = px_; plat = py_; }   // ecef_to_model, delay.py:253
                    // all-pixels z-clamp of the very first / very last sample (delay.py:306-311): when it applies every
                    // pixel is below (above) the cube, so "set to zmin" == max(ph, zmin); the bounds are wave-uniform
                    if (clamp_any) {
                        const double zfloor = (clamp_lo && k == k0 && j == 0) ? c.z_lo : -__builtin_huge_val();
                        const double zceil = (clamp_hi && k == K - 1 && j == np - 1) ? c.z_hi : __builtin_huge_val();
                        ph = fmin(fmax(ph, zfloor), zceil);
                    }
                    double vw, vh;
                    sample_cube(c, m.ax, plat, plon, ph, kz, vw, vh);                   // delay.py:298,319
                    const double wt = ((j == 0) | (j == np - 1)) ? 0.5 * segw : segw;     // delay.py:314-315
                    acc_w = fma(wt, vw, acc_w); acc_h = fma(wt, vh, acc_h);               // delay.py:323
                    vw_top = vw; vh_top = vh;                                             // after the loop: value at j = np-1
                }
            }
        }
        if (active && mine) { const auto& oa = Pk(); const int64_t o = (int64_t)sl * oa.n + i; oa.wet[o] = acc_w + poison; oa.hyd[o] = acc_h + poison; }
    }
}

}  // namespace rdr
