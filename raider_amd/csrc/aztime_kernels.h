// Azimuth-time-grid temporal interpolation in one pass: orbit -> per-voxel acquisition time -> weights -> combined cubes.
// Part of libraider_hip.so (single translation unit: included by raider_hip.hip after cube_kernels.h and orbit_kernels.h).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "cube_kernels.h"
#include "orbit_kernels.h"

using namespace rdr;

// The 'azimuth_time_grid' branch of combine_weather_files (cli/raider.py:791-832) per voxel of the model grid, nothing materialised:
//   get_time_grid_for_aztime_interp (:891-916)   lat2d / lon2d broadcast over z, lla2ecef
//   get_azimuth_time_grid (s1_azimuth_timing.py:90-147)   zero-Doppler time + one-way range delay, truncated to milliseconds
//   get_inverse_weights_for_dates (:326-399)     time_weights_kernel's expressions
//   ds_out[var] = sum(w_i * ds_i[var]) (:817-819)   blend_weighted_kernel's expressions, for the pointwise and the total cubes
// One lane per voxel of the device layout (y, x, z), z fastest.  lat2d / lon2d: [ny][nx] in the cubes' (ascending) axis order.
// tgrid (may be NULL): [nz][ny][nx] seconds relative to dates[0].  flags: bit 0 = a voxel's solve failed or left the orbit span
// (its outputs are NaN), bit 2 = some date lay inside the window at some voxel.
constexpr double AZTIME_SPEED_OF_LIGHT = 299792458.0;       // isce3.core.speed_of_light (s1_azimuth_timing.py:138-139)

struct AzTimeArgs {
    const double *st, *sp, *sv; int nsv;                     // state vectors (device)
    const double *lat2d, *lon2d, *zs;
    int64_t ny, nx, nz;
    CubeSet P, T;                                            // pointwise / total epochs; v[0] == NULL: that set is absent
    DateSet D;
    long long offset_us;                                     // (orbit epoch truncated to ms) - dates[0], microseconds
    double2 *out_p, *out_t;
    double* tgrid;
    int* flags;
};

template <typename TP2, typename TT2>
__global__ __launch_bounds__(256) void aztime_blend_kernel(AzTimeArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char orbit_smem[];
    const OrbitTables T = orbit_tables_build(orbit_smem, A.st, A.sp, A.sv, A.nsv);
    const int64_t total = A.ny * A.nx * A.nz;
    const bool has_p = A.P.v[0] != nullptr, has_t = A.T.v[0] != nullptr;
    int bits = 0;
    for (int64_t o = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; o < total; o += (int64_t)gridDim.x * blockDim.x) {
        const int64_t iz = o % A.nz, ix = (o / A.nz) % A.nx, iy = o / (A.nz * A.nx);
        double tx, ty, tz;
        lla2ecef(A.lat2d[iy * A.nx + ix], A.lon2d[iy * A.nx + ix], A.zs[iz], tx, ty, tz);
        double az, pos[3], t = qnan();
        if (orbit_zero_doppler(T, tx, ty, tz, 1.0e-7, 100, az, pos)) {
#pragma clang fp contract(off)
            const double dx = pos[0] - tx, dy = pos[1] - ty, dz = pos[2] - tz;
            const double rg = sqrt(dx * dx + dy * dy + dz * dz);
            const double sec = floor((az + rg / AZTIME_SPEED_OF_LIGHT) * 1e3) / 1e3;       // s1_azimuth_timing.py:138-141, datetime64[ms]
            const long long tick = llrint(sec * 1e3);
            t = (double)(tick * 1000 + A.offset_us) / 1e6;                                 // relative to dates[0]
        } else bits |= 1;
        if (A.tgrid) A.tgrid[(iz * A.ny + iy) * A.nx + ix] = t;
        // time_weights_kernel: m_d = (1 / (|t - date_d| + reg)) * [|t - date_d| <= window], w_d = m_d / sum(m)
        double msum = 0.0;
        for (int d = 0; d < A.D.nd; ++d) {
            const double diff = fabs(t - A.D.date[d]);
            const bool in = diff <= A.D.window;
            if (in) bits |= 4;
            const double m = (1.0 / (diff + A.D.reg)) * (in ? 1.0 : 0.0);
            msum += m;
        }
        double pw = 0.0, ph = 0.0, tw = 0.0, th = 0.0;
        for (int d = 0; d < A.D.nd; ++d) {
            const double diff = fabs(t - A.D.date[d]);
            const double m = (1.0 / (diff + A.D.reg)) * (diff <= A.D.window ? 1.0 : 0.0);
            const double wd = m / msum;
            // blend_weighted_kernel: ((0 + w0 a0) + w1 a1) + ... in f64, products and sums rounded separately
            if (has_p) {
                const TP2 v = reinterpret_cast<const TP2*>(A.P.v[d])[o];
                {
#pragma clang fp contract(off)
                    const double a = wd * (double)v.x, b = wd * (double)v.y;
                    pw = pw + a; ph = ph + b;
                }
            }
            if (has_t) {
                const TT2 v = reinterpret_cast<const TT2*>(A.T.v[d])[o];
                {
#pragma clang fp contract(off)
                    const double a = wd * (double)v.x, b = wd * (double)v.y;
                    tw = tw + a; th = th + b;
                }
            }
        }
        if (has_p) { double2 r; r.x = pw; r.y = ph; A.out_p[o] = r; }
        if (has_t) { double2 r; r.x = tw; r.y = th; A.out_t[o] = r; }
    }
    if (bits) atomicOr(A.flags, bits);
}
