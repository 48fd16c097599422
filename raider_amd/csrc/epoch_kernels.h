// Pass 2 of a time series (rdr_raytrace_slices_epochs, rdr_raytrace_epochs): E weather epochs on ONE ray geometry, marched together.
//
//   march_epochs_kernel   march_kernel (raider_kernels.h) with E cubes.  Everything but the entry point is march_kernel's own code: the
//                         slice partition, the tile mapping, the ray record, the no-check proof - and the two level loops
//                         (march_slice_levels, PR = false: a series of height slices; march_ray_height_levels, PR = true:
//                         rdr_raytrace_epochs with rays->hts), function templates over the number of cubes that march_kernel calls
//                         with E = 1 and this kernel with its E.  Per sample the shared part - the ray polynomials, the x / y cell
//                         search, the z window, the corner offset - runs once; then E corner-pair gathers (independent of each
//                         other: the ILP the one-epoch marcher lacks) and E (wet, hydro) accumulators.
//
// Per epoch the instructions are march_kernel's own, from the same source lines: sample_finish_lerp on the same weights, the same
// trapezoid weights, the same accumulation order - so epoch e's delays are bit for bit what rdr_raytrace_slices / rdr_raytrace give on
// cube e.  Generic rays (record field WS_SCALE == 0) are left to march_kernel<T2, true>, launched once per epoch on the same records.
// The f64 LDS staging of march_kernel (STAGED) is not carried over: with E gathers per sample in flight the direct loads are what the
// stacked loop needs.
//
//   interp_points_epochs_kernel  the point gather of interp_points_kernel with E cubes: a date series at query points
//                         (rdr_interp3_project_epochs, rdr_point_delays_epochs), at the end of this file.  Its body is gather_points
//                         (cube_kernels.h), the one every point gather shares.
//
// Layout: pointer per epoch.  The E cubes share shape, axes and projection (checked on the host), so one element offset serves
// every epoch and the corner-pair reads of an epoch are exactly the single-epoch kernel's (16 B / 32 B contiguous per corner pair).
#pragma once
#include "raider_kernels.h"
#include "cube_kernels.h"

namespace rdr {

constexpr int EPOCHS_MAX = 4;          // epochs per stacked launch (DESIGN.md "Time series")

// Occupancy per (dtype, E, PR): the highest at which the compiler's resource report shows no scratch (DESIGN.md "Time series", 5d).
// Slice loop: at four waves per SIMD f32 / E = 2 spills 48-80 B per lane, at three f32 / E = 4 48-112 B and f64 / E = 2 16-32 B.
// Per-ray-height loop: one step up f32 / E = 2 spills 64-100 B per lane, f32 / E = 4 88-96 B, f64 / E = 2 36-60 B; f64 / E = 4 needs
// 8 B at two waves per SIMD on REGULAR grids (256 VGPRs), so it is built for one - and the driver does not use it by default (epoch_group).
template <typename T2, int E, bool PR>
struct EpochWaves {
    static constexpr int value = PR ? (sizeof(T2) == 8 ? (E <= 2 ? 3 : 2) : (E <= 2 ? 2 : 1)) : ((sizeof(T2) == 8 && E <= 2) ? 3 : 2);
};

// GRID as in march_kernel: 1 REGULAR (exact axes, 32-bit offsets), 2 TABLES (nearly uniform axes, 32-bit offsets), 0 run-time flags.
// PR as in march_kernel: per-ray origin heights (P.ht_ray; one slice) - REGULAR or run-time flags, the two the one-epoch per-ray-height
// marcher is launched with.
// Outputs: epoch e of slice-major ray index o at P.wet[e * estride + o] / P.hyd[e * estride + o].
template <typename T2, int E, int GRID, bool PR>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(EpochWaves<T2, E, PR>::value, EpochWaves<T2, E, PR>::value)))
void march_epochs_kernel(CubeView<T2> c_in, EpochCubes<T2, E> ev, RayParams P, int64_t estride) {
    static_assert(!PR || GRID == 0 || GRID == 1, "per-ray heights: REGULAR or run-time flags");
    constexpr bool REGULAR = GRID == 1;
    CubeView<T2> c = c_in;
    if (REGULAR) { c.exact_y = 1; c.exact_x = 1; c.small = 1; }
    if (GRID == 2) { c.exact_y = 0; c.exact_x = 0; c.uni_y = 1; c.uni_x = 1; c.small = 1; }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const RaySmem m = carve_smem(smem_raw, c.ny, c.nx, c.nz, c.exact_y, c.exact_x);
    fill_axes(c, m);
    int K = 0, slice = -1;
    double poison = 0.0;
    bool clamp_lo = false, clamp_hi = false;
    TileWalk walk(P.tile_count, P.tile_ctr, m.K + 2);
    int64_t lt;
    while (walk.next(P.tile_count, lt)) {
        const int64_t tg = P.tile_begin + lt;
        const int sl = (int)(tg / P.tiles_per_slice);
        const int64_t t = tg - (int64_t)sl * P.tiles_per_slice;
        if (sl != slice) {                                 // the slice's level table and partition (packed records: the slice loop only)
            slice = sl;
            K = fill_levels(c.nz, m, P.hts ? P.hts[sl] : P.ht, P.zref);
            const SlicePartition part = fill_partition(P, m, sl, K);
            poison = part.poison; clamp_lo = part.clamp_lo; clamp_hi = part.clamp_hi;
        }
        int tl = threadIdx.x;
        asm volatile("" : "+v"(tl));
        int64_t i; bool active;
        tile_ray(P, t, tl, i, active);
        const double* w = P.ws + (lt * BLOCK + tl);
        const int64_t ns = P.nslots;
        const double scale_rec = w[(int64_t)WS_SCALE * ns];
        const bool mine = !active || scale_rec != 0.0;     // light rays (and tile padding); generic rays: march_kernel<T2, true>
        // per-ray heights: the ray's first level of the slice table, found exactly as pass 1 found it (idle lanes: none)
        int k0 = 0; double lo_first = K > 0 ? m.lo[0] : 0.0;
        if constexpr (PR) k0 = (active && mine) ? first_level(m.ax.ez, c.nz, m.lo, m.hi, m.kz, K, P.ht_ray[i], lo_first) : K;
        double acc_w[E], acc_h[E];
#pragma unroll
        for (int e = 0; e < E; ++e) { acc_w[e] = 0.0; acc_h[e] = 0.0; }
        RayPoly q;
        double xc[PX];
        load_ray_record(w, ns, q, xc);
        const double scale = scale_rec;
        const double u0r = w[(int64_t)WS_U0 * ns], u1r = w[(int64_t)WS_U1 * ns];
        const unsigned long long live = __builtin_amdgcn_ballot_w64(active && mine);
        const LevelRec* const lev = PR ? nullptr : P.lev + (int64_t)__builtin_amdgcn_readfirstlane(sl) * (c.nz + 1);     // (per tile: march_kernel)
        auto run = [&](auto nochk) {
            constexpr bool NC = decltype(nochk)::value;
            if constexpr (PR) march_ray_height_levels<T2, E, NC>(c, ev, m, q, xc, u0r, u1r, K, k0, lo_first, clamp_lo, clamp_hi, acc_w, acc_h);
            else march_slice_levels<T2, E, NC>(c, ev, m, q, xc, lev, u0r, u1r, K, clamp_lo, clamp_hi, live, acc_w, acc_h);
        };
        // the wave-wide no-check proof (lane_nocheck): bounds of the cell search from the polynomial coefficients
        bool lane_safe = false;
        if (REGULAR) lane_safe = lane_nocheck(u0r, u1r, active, mine, q, xc, c.ny, c.nx);
        if (REGULAR && __all(lane_safe)) run(std::integral_constant<bool, true>{});
        else run(std::integral_constant<bool, false>{});
        if (active && scale_rec != 0.0) {
            const int64_t o = (int64_t)sl * P.n + i;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double aw = acc_w[e] * scale, ah = acc_h[e] * scale;
                P.wet[e * estride + o] = aw + poison; P.hyd[e * estride + o] = ah + poison;
            }
        }
    }
}

// ---- a date series at query points (rdr_interp3_project_epochs, rdr_point_delays_epochs) ------------------------------------
// interp_points_epochs_kernel: interp_points_kernel (cube_kernels.h) with E cubes of one grid - the same body, gather_points, with E plain
// corner sources, one per epoch's base pointer.  One query point per lane; per point the bounds test, the three cell searches, the three
// divisions and the eight weights run ONCE; then per epoch the eight corner loads and the corner sum: epoch e's values are bit for bit
// what interp_points_kernel gives on cube e, because it is the same code.  The plain (y, x, z) layout only: no corner quads, no paired
// columns.
// Outputs are epoch-major: wet[e * estride + i], hyd[e * estride + i] (estride >= n: a chunk of a pipelined call keeps the full stride).
// The projection is PointQuery::store's: pmode 0..3; pstride 0: one divisor proj[i] for every epoch, else proj[e * pstride + i].
template <typename T2, int E>
__global__ __launch_bounds__(256) void interp_points_epochs_kernel(CubeView<T2> c, EpochCubes<T2, E> ev, PointQuery Q, int64_t pstride, int64_t n, int64_t estride,
                                                                   double* __restrict__ wet, double* __restrict__ hyd, int axes_in_lds) {
    PlainCorners<T2> src[E];
#pragma unroll
    for (int e = 0; e < E; ++e) src[e].v = ev.v[e];
    gather_points<E>(c, src, Q, pstride, n, estride, wet, hyd, axes_in_lds);
}

}  // namespace rdr
