// raster_kernels.h - georeferenced rasters on the device: DEM sampling at query points and the bounds of lat / lon rasters.
//
//   raster_sample_kernel<T, METHOD>   interpolateDEM / interpolate_elevation [interpolator.py:133-184]: one query point per lane,
//                                     a north-up raster in its file element type (int16 / f32 / f64), f64 coordinates in, f64 out
//   raster_bounds_kernel<T>           rio_stats' minimum / maximum [utilFcns.py:213-241] of up to two equal-length rasters as
//   raster_bounds_final_kernel        bounds_from_latlon_rasters [llreader.py:397-420] asks for them: one partial per workgroup,
//                                     then one workgroup over the partials; no floating-point atomics, so the same bytes every run
//
// Both are memory bound and need a handful of registers; there is nothing to tile and nothing for the matrix cores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdr {

enum { RASTER_NEAREST = 0, RASTER_LINEAR = 1 };

struct RasterGeo {
    int64_t height, width;
    double x0, dx, y0, dy;      // GDAL's gt[0], gt[1], gt[3], gt[5] (gt[2] == gt[4] == 0: the entry point refuses a rotation)
};

__device__ __forceinline__ double raster_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

template <typename T>
__device__ __forceinline__ double raster_value(const T* __restrict__ r, int64_t idx, int has_nodata, double nodata) {
    const double v = (double)r[idx];
    return (has_nodata && v == nodata) ? raster_nan() : v;
}

// Centre of pixel k on the ASCENDING copy of an axis (scipy and xarray sort a descending coordinate before they interpolate):
// origin + (j + 0.5) * step with j = k for step > 0 and j = n - 1 - k for step < 0.  Product and sum are rounded separately (no fused
// multiply-add), so that a host restatement in NumPy reproduces the node - and with it the weight - bit for bit.
__device__ __forceinline__ double raster_centre(double origin, double step, int64_t n, int64_t k) {
    const int64_t j = step > 0.0 ? k : n - 1 - k;
    return __dadd_rn(origin, __dmul_rn((double)j + 0.5, step));
}

// scipy's find_indices on that ascending axis for a coordinate inside the hull: g[k] <= v < g[k+1], the last cell closed.
__device__ __forceinline__ int64_t raster_cell(double origin, double step, int64_t n, double v, double g0) {
    int64_t k = (int64_t)floor((v - g0) / fabs(step));
    k = k < 0 ? 0 : (k > n - 2 ? n - 2 : k);
    while (k > 0 && v < raster_centre(origin, step, n, k)) --k;                  // (the guess is off by at most one cell: rounding of the quotient)
    while (k < n - 2 && v >= raster_centre(origin, step, n, k + 1)) ++k;
    return k;
}

template <typename T, int METHOD>
__global__ __launch_bounds__(256) void raster_sample_kernel(const T* __restrict__ raster, RasterGeo g, const double* __restrict__ x,
                                                            const double* __restrict__ y, int64_t n, int has_nodata, double nodata,
                                                            double* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double px = x[i], py = y[i];
        double v = raster_nan();
        if (METHOD == RASTER_NEAREST) {
            // rasterio.transform.rowcol with its default op = floor (interpolator.py:173): the pixel whose cell holds the point.  A NaN
            // coordinate fails both comparisons.
            const double col = floor((px - g.x0) / g.dx);
            const double row = floor((py - g.y0) / g.dy);
            if (col >= 0.0 && col < (double)g.width && row >= 0.0 && row < (double)g.height)
                v = raster_value(raster, (int64_t)row * g.width + (int64_t)col, has_nodata, nodata);
        } else {
            // bilinear on pixel-centre coordinates (da_dem.interp(y=, x=), interpolator.py:149); NaN outside the hull of the centres,
            // the last centre itself inside
            const double gx0 = raster_centre(g.x0, g.dx, g.width, 0), gx1 = raster_centre(g.x0, g.dx, g.width, g.width - 1);
            const double gy0 = raster_centre(g.y0, g.dy, g.height, 0), gy1 = raster_centre(g.y0, g.dy, g.height, g.height - 1);
            if (px >= gx0 && px <= gx1 && py >= gy0 && py <= gy1) {
                const int64_t kx = raster_cell(g.x0, g.dx, g.width, px, gx0);
                const int64_t ky = raster_cell(g.y0, g.dy, g.height, py, gy0);
                const double xa = raster_centre(g.x0, g.dx, g.width, kx), xb = raster_centre(g.x0, g.dx, g.width, kx + 1);
                const double ya = raster_centre(g.y0, g.dy, g.height, ky), yb = raster_centre(g.y0, g.dy, g.height, ky + 1);
                const double tx = (px - xa) / (xb - xa);
                const double ty = (py - ya) / (yb - ya);
                // back to file order: row / column of ascending node k
                const int64_t c0 = g.dx > 0.0 ? kx : g.width - 1 - kx, c1 = g.dx > 0.0 ? kx + 1 : g.width - 2 - kx;
                const int64_t r0 = g.dy > 0.0 ? ky : g.height - 1 - ky, r1 = g.dy > 0.0 ? ky + 1 : g.height - 2 - ky;
                const double v00 = raster_value(raster, r0 * g.width + c0, has_nodata, nodata);
                const double v01 = raster_value(raster, r0 * g.width + c1, has_nodata, nodata);
                const double v10 = raster_value(raster, r1 * g.width + c0, has_nodata, nodata);
                const double v11 = raster_value(raster, r1 * g.width + c1, has_nodata, nodata);
                // the weight order of corner_weights / corner_sum (raider_kernels.h) on two axes: weight = (1 * wy) * wx, corners in (y, x) order, 0 + sum
                const double wy0 = 1.0 - ty, wx0 = 1.0 - tx;
                double s = 0.0;
                s += v00 * (wy0 * wx0);
                s += v01 * (wy0 * tx);
                s += v10 * (ty * wx0);
                s += v11 * (ty * tx);
                v = s;
            }
        }
        out[i] = v;
    }
}

// ---- bounds ------------------------------------------------------------------------------------------------------------------------
struct RasterRange {
    double lo, hi;
    int64_t count;      // valid elements: neither NaN nor the no-data value
};

__device__ __forceinline__ void range_take(RasterRange& r, double v, int has_nodata, double nodata) {
    if (v == v && !(has_nodata && v == nodata)) {
        r.lo = v < r.lo ? v : r.lo;
        r.hi = v > r.hi ? v : r.hi;
        ++r.count;
    }
}

__device__ __forceinline__ void range_merge(RasterRange& r, double lo, double hi, int64_t count) {
    r.lo = lo < r.lo ? lo : r.lo;
    r.hi = hi > r.hi ? hi : r.hi;
    r.count += count;
}

// One lane's share of one raster.  The body goes in 16-byte loads (8 int16 / 4 f32 / 2 f64 per lane, 1 KiB per wave instruction);
// the elements before the first 16-byte boundary and behind the last whole vector are taken one per lane.
template <typename T>
__device__ __forceinline__ void range_scan(const T* __restrict__ p, int64_t n, int has_nodata, double nodata, RasterRange& r) {
    constexpr int V = 16 / (int)sizeof(T);
    struct alignas(16) Pack { T v[V]; };
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
    int64_t head = (int64_t)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) / sizeof(T));
    head = head < n ? head : n;
    for (int64_t i = tid; i < head; i += nthreads) range_take(r, (double)p[i], has_nodata, nodata);
    const int64_t nvec = (n - head) / V;
    const Pack* pv = reinterpret_cast<const Pack*>(p + head);
    for (int64_t i = tid; i < nvec; i += 4 * nthreads) {        // four independent loads in flight per lane before the first comparison
        Pack c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * nthreads < nvec) c[u] = pv[i + u * nthreads];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * nthreads < nvec) {
#pragma unroll
                for (int j = 0; j < V; ++j) range_take(r, (double)c[u].v[j], has_nodata, nodata);
            }
    }
    const int64_t done = head + nvec * V;
    for (int64_t i = done + tid; i < n; i += nthreads) range_take(r, (double)p[i], has_nodata, nodata);
}

// wave (shuffles) -> workgroup (LDS); the result is valid in thread 0.  blockDim.x == 256.
__device__ __forceinline__ void range_block_reduce(RasterRange (&r)[2], double (*lds)[6]) {
    for (int k = 0; k < 2; ++k)
        for (int off = 32; off > 0; off >>= 1)
            range_merge(r[k], __shfl_down(r[k].lo, off, 64), __shfl_down(r[k].hi, off, 64), (int64_t)__shfl_down((long long)r[k].count, off, 64));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 2; ++k) { lds[wave][3 * k] = r[k].lo; lds[wave][3 * k + 1] = r[k].hi; lds[wave][3 * k + 2] = (double)r[k].count; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w)
            for (int k = 0; k < 2; ++k) range_merge(r[k], lds[w][3 * k], lds[w][3 * k + 1], (int64_t)lds[w][3 * k + 2]);
}

// Stage 1: partial[blockIdx.x][6] = (lo, hi, count) of a, then of b (b == NULL: the empty range).  Counts travel as doubles: exact to 2^53.
template <typename T>
__global__ __launch_bounds__(256) void raster_bounds_kernel(const T* __restrict__ a, const T* __restrict__ b, int64_t n, int has_nodata,
                                                            double nodata, double* __restrict__ partial) {
    __shared__ double lds[4][6];
    RasterRange r[2] = {{INFINITY, -INFINITY, 0}, {INFINITY, -INFINITY, 0}};
    range_scan(a, n, has_nodata, nodata, r[0]);
    if (b) range_scan(b, n, has_nodata, nodata, r[1]);
    range_block_reduce(r, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < 2; ++k) {
            partial[(int64_t)blockIdx.x * 6 + 3 * k] = r[k].lo;
            partial[(int64_t)blockIdx.x * 6 + 3 * k + 1] = r[k].hi;
            partial[(int64_t)blockIdx.x * 6 + 3 * k + 2] = (double)r[k].count;
        }
}

// Stage 2 (one workgroup): out6 = (min, max, valid count) of a, then of b; min and max of a raster without a valid element are NaN.
__global__ __launch_bounds__(256) void raster_bounds_final_kernel(const double* __restrict__ partial, int nparts, double* __restrict__ out6) {
    __shared__ double lds[4][6];
    RasterRange r[2] = {{INFINITY, -INFINITY, 0}, {INFINITY, -INFINITY, 0}};
    for (int i = threadIdx.x; i < nparts; i += blockDim.x)
        for (int k = 0; k < 2; ++k) range_merge(r[k], partial[(int64_t)i * 6 + 3 * k], partial[(int64_t)i * 6 + 3 * k + 1], (int64_t)partial[(int64_t)i * 6 + 3 * k + 2]);
    range_block_reduce(r, lds);
    if (threadIdx.x == 0)
        for (int k = 0; k < 2; ++k) {
            out6[3 * k] = r[k].count ? r[k].lo : raster_nan();
            out6[3 * k + 1] = r[k].count ? r[k].hi : raster_nan();
            out6[3 * k + 2] = (double)r[k].count;
        }
}

}  // namespace rdr
