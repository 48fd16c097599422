// Pass 2 of a time series (rdr_raytrace_slices_epochs, rdr_raytrace_epochs): E weather epochs on ONE ray geometry, marched together.
//
//   march_epochs_kernel   march_kernel (raider_kernels.h) with E cubes, built from the same parts: the slice partition, the tile
//                         mapping, the ray record and the no-check proof are march_kernel's own functions; per sample the shared
//                         part - the ray polynomials, the x / y cell search, the z window, the corner offset - runs once; then E
//                         corner-pair gathers (independent of each other: the ILP the one-epoch marcher lacks) and E (wet, hydro)
//                         accumulators.  Its two level loops are march_kernel's two: the light slice loop (PR = false; a series of
//                         height slices) and the per-ray-height loop (PR = true; rdr_raytrace_epochs with rays->hts).
//
// Per epoch the arithmetic is march_kernel's own: sample_finish_lerp on the same weights, the same trapezoid weights, the same
// accumulation order - so epoch e's delays are bit for bit what rdr_raytrace_slices / rdr_raytrace give on cube e.  Generic rays (record field
// WS_SCALE == 0) are left to march_kernel<T2, true>, launched once per epoch on the same records.  The f64 LDS staging of
// march_kernel (STAGED) is not carried over: with E gathers per sample in flight the direct loads are what the stacked loop needs.
//
//   interp_points_epochs_kernel  the point gather of interp_points_kernel (cube_kernels.h) with E cubes: a date series at query points
//                         (rdr_interp3_project_epochs, rdr_point_delays_epochs), at the end of this file.
//
// Layout: pointer per epoch.  The E cubes share shape, axes and projection (checked on the host), so one element offset serves
// every epoch and the corner-pair reads of an epoch are exactly the single-epoch kernel's (16 B / 32 B contiguous per corner pair).
#pragma once
#include "raider_kernels.h"
#include "cube_kernels.h"

namespace rdr {

constexpr int EPOCHS_MAX = 4;          // epochs per stacked launch (DESIGN.md "Time series")

template <typename T2, int E>
struct EpochCubes { const T2* v[E]; };

// E samples that share their cell and weights: one set of corners per epoch
template <typename T2, int E>
struct PendingSampleE {
    T2 v[E][8];
    double ty, tx, tz;
};

// gather_corners for E cubes of one shape: cell_xy once, the element offset once, E x 4 corner-pair loads
template <typename T2, int E, bool IDX, bool NOCHECK>
__device__ __forceinline__ void gather_corners_e(const CubeView<T2>& c, const EpochCubes<T2, E>& ev, const AxisTabs& m, double y, double x, int iz,
                                                 PendingSampleE<T2, E>& s) {
    int iy, ix;
    cell_xy<IDX, NOCHECK>(m.ey, c.ny, y, c.y_lo, c.y_hi, c.inv_dy, c.exact_y, c.uni_y, iy, s.ty);
    cell_xy<IDX, NOCHECK>(m.ex, c.nx, x, c.x_lo, c.x_hi, c.inv_dx, c.exact_x, c.uni_x, ix, s.tx);
    if (c.small) {
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
            const SlicePartition part = fill_partition<!PR>(P, m, c.nz, sl, K);
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
        const unsigned long long live = __builtin_amdgcn_ballot_w64(active && mine);
        auto finish = [&](const PendingSampleE<T2, E>& s, double wv) {
#pragma unroll
            for (int e = 0; e < E; ++e) {
                PendingSample<T2> one;
#pragma unroll
                for (int j = 0; j < 8; ++j) one.v[j] = s.v[e][j];
                one.ty = s.ty; one.tx = s.tx; one.tz = s.tz;
                double vw, vh;
                sample_finish_lerp(one, vw, vh);
                acc_w[e] = fma(wv, vw, acc_w[e]); acc_h[e] = fma(wv, vh, acc_h[e]);
            }
        };
        auto run = [&](auto nochk) {
            constexpr bool NC = decltype(nochk)::value;
            if constexpr (PR) {
                // The per-ray-height loop of march_kernel<T2, false, GRID, true> with E cubes.  The level schedule (k, j) stays
                // slice-uniform; a lane joins it at its own first level k0 with its own first sample, the loop starts at the wave's
                // lowest k0.  Per sample the polynomials, the z cell, cell_xy and the element offset run once, then E corner-pair
                // gathers and E accumulator pairs.
                // a level's top sample / the ray's first sample: the two-entry z window (sample_issue MODE 1)
                auto issue_top = [&](double us, int zbase, bool floor_it, bool ceil_it, PendingSampleE<T2, E>& s) {
                    double ph = poly5(q.h, us);
                    const double plat = poly5(q.lat, us), plon = poly5(q.lon, us);
                    if (floor_it) { asm volatile("" ::: "memory"); ph = fmax(ph, c.z_lo); }
                    if (ceil_it) { asm volatile("" ::: "memory"); ph = fmin(ph, c.z_hi); }
                    int iz;
                    window2_cell(m.ax.ez, c.nz, ph, zbase, c.nz >= 4, iz, s.tz);
                    gather_corners_e<T2, E, true, NC>(c, ev, m.ax, plat, plon, iz, s);
                };
                int kmin = k0;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) kmin = min(kmin, __shfl_xor(kmin, off, 64));
                kmin = __builtin_amdgcn_readfirstlane(kmin);
                // every lane's FIRST sample (the bottom of its own first level) in one evaluation for the whole wave
                const bool has = k0 < K;
                const int kf = has ? k0 : 0;
                double u_k = has ? w[(int64_t)WS_U0 * ns] : 0.0, u_last = has ? w[(int64_t)WS_U1 * ns] : 0.0;
                double du = u_last - u_k;
                if (K > 0) {
                    const int kzf = m.kz[kf];
                    PendingSampleE<T2, E> s;
                    issue_top(fma(0.0 * m.step[kf], du, u_k), window2_base(c.nz, kzf - ((lo_first <= m.ax.ez[kzf].x) ? 1 : 0)), clamp_lo, false, s);
                    if (has) finish(s, m.hs[kf] * fabs(du));
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
                        for (int j = 1; j < np - 1; ++j) {      // strictly inside model interval kz (sample_issue MODE 2)
                            PendingSampleE<T2, E> s;
                            const double us = fma((double)j * step, du, u_k);
                            const double ph = poly5(q.h, us);
                            const double plat = poly5(q.lat, us), plon = poly5(q.lon, us);
                            const double2 e0 = m.ax.ez[kz];
                            int iz = kz;
                            s.tz = (ph - e0.x) * e0.y;
                            if (!(s.tz >= 0.0) || !(s.tz <= 1.0)) cell_exact(m.ax.ez, c.nz, ph, iz, s.tz);   // rare
                            gather_corners_e<T2, E, true, NC>(c, ev, m.ax, plat, plon, iz, s);
                            finish(s, w_mid);
                        }
                        PendingSampleE<T2, E> top;
                        issue_top(u_k + du, zbase, false, clamp_hi && !more, top);
                        double du1 = 0.0;
                        double w_top = hs * fabs(du);
                        if (more) {
                            const double t2 = poly7(xc, m.xv[k + 1]);
                            du1 = t2 - u_last; u_last = t2;
                            w_top = fma(m.hs[k + 1], fabs(du1), w_top);
                        }
                        finish(top, w_top);
                        u_k += du; du = du1;
                    }
                }
            } else {
                // The light slice loop of march_kernel with E cubes (packed level records through one LDS address register).
                typedef __attribute__((address_space(3))) const LevelRec LdsRec;
                int la = (int)(size_t)m.lev;
                asm volatile("" : "+v"(la));
                const LdsRec* rec = (const LdsRec*)(size_t)(unsigned)la;
                int npkz = __builtin_amdgcn_readfirstlane(rec->npkz);
                int np = npkz & 0x1ffff, kz = npkz >> 17;
                double hs = rec->hs;
                double u_k = w[(int64_t)WS_U0 * ns];
                double u_last = w[(int64_t)WS_U1 * ns];
                double du = u_last - u_k;
                if (K > 0) {                                   // the ray's very first sample (march_kernel: issue_top with MODE 1)
                    PendingSampleE<T2, E> s;
                    const double us = fma(0.0 * rec->step, du, u_k);
                    double ph = poly5(q.h, us);
                    const double plat = poly5(q.lat, us), plon = poly5(q.lon, us);
                    if (clamp_lo) { asm volatile("" ::: "memory"); ph = fmax(ph, c.z_lo); }
                    int iz;
                    window2_cell(m.ax.ez, c.nz, ph, window2_base(c.nz, kz - ((m.lo[0] <= m.ax.ez[kz].x) ? 1 : 0)), c.nz >= 4, iz, s.tz);
                    gather_corners_e<T2, E, true, NC>(c, ev, m.ax, plat, plon, iz, s);
                    finish(s, hs * fabs(du));
                }
#pragma unroll 1
                for (int k = 0; k < K; ++k) {
                    const int zbase = window2_base(c.nz, kz);
                    const bool more = k + 1 < K;
                    const double w_mid = (2.0 * hs) * fabs(du);
                    if (np > 2) {
                        const double step = rec->step, gk = rec->gk, rk = rec->rk;
#pragma unroll 1
                        for (int j = 1; j < np - 1; ++j) {
                            PendingSampleE<T2, E> s;
                            const double us = fma((double)j * step, du, u_k);
                            const double ph = poly5(q.h, us), plat = poly5(q.lat, us), plon = poly5(q.lon, us);
                            int iz = kz;
                            s.tz = (ph - gk) * rk;
                            if (!(s.tz >= 0.0) || !(s.tz <= 1.0)) cell_exact(m.ax.ez, c.nz, ph, iz, s.tz);   // rare
                            gather_corners_e<T2, E, true, NC>(c, ev, m.ax, plat, plon, iz, s);
                            finish(s, w_mid);
                        }
                    }
                    PendingSampleE<T2, E> top;
                    {
                        const double us = u_k + du;
                        double ph = poly5(q.h, us);
                        const double plat = poly5(q.lat, us), plon = poly5(q.lon, us);
                        if (clamp_hi && !more) { asm volatile("" ::: "memory"); ph = fmin(ph, c.z_hi); }
                        const double d = ph - rec->zmid;
                        int iz; bool ok;
                        if (__builtin_expect((__builtin_amdgcn_ballot_w64(!(d >= 0.0)) & live) == 0ULL, 1)) {
                            iz = zbase + 1;
                            top.tz = d * rec->r1;
                            ok = top.tz <= 1.0;
                        } else {
                            double ds = d;
                            asm volatile("" : "+v"(ds));
                            const bool up = ds >= 0.0;
                            iz = zbase + (int)up;
                            top.tz = fma(ds, up ? rec->r1 : rec->r0, up ? 0.0 : 1.0);
                            ok = (top.tz >= 0.0) & (top.tz <= 1.0);
                        }
                        if (!(ok & (c.nz >= 4))) cell_exact(m.ax.ez, c.nz, ph, iz, top.tz);                  // rare
                        gather_corners_e<T2, E, true, NC>(c, ev, m.ax, plat, plon, iz, top);
                    }
                    const double t2 = poly7(xc, rec[1].xv);
                    const double du1 = t2 - u_last, hs1 = rec[1].hs;
                    u_last = t2;
                    const double w_top = fma(hs1, fabs(du1), hs * fabs(du));
                    npkz = __builtin_amdgcn_readfirstlane(rec[1].npkz);
                    finish(top, w_top);
                    u_k += du; du = du1; hs = hs1;
                    np = npkz & 0x1ffff; kz = npkz >> 17;
                    ++rec;
                }
            }
        };
        // the wave-wide no-check proof (lane_nocheck): bounds of the cell search from the polynomial coefficients
        bool lane_safe = false;
        if (REGULAR) lane_safe = lane_nocheck(w[(int64_t)WS_U0 * ns], w[(int64_t)WS_U1 * ns], active, mine, q, xc, c.ny, c.nx);
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
// interp_points_epochs_kernel: interp_points_kernel (cube_kernels.h) with E cubes of one grid.  One query point per lane; per point the
// bounds test, the three cell searches, the three divisions, the eight weights and the element offset run ONCE; then per epoch the eight
// corner loads from that epoch's own base pointer and trilinear<>'s sum (raider_kernels.h), in its corner order and operation order: the
// same source expressions, so the compiler contracts them into the same fma chain - epoch e's values are bit for bit what
// interp_points_kernel gives on cube e.  The plain (y, x, z) layout only: no corner quads, no paired columns.
// Outputs are epoch-major: wet[e * estride + i], hyd[e * estride + i] (estride >= n: a chunk of a pipelined call keeps the full stride).
// The projection is PointQuery::store's: pmode 0..3; pstride 0: one divisor proj[i] for every epoch, else proj[e * pstride + i]
// (Conventional with an orbit file: setTime per date, so the divisor may differ by date).
template <typename T2, int E>
__global__ __launch_bounds__(256) void interp_points_epochs_kernel(CubeView<T2> c, EpochCubes<T2, E> ev, PointQuery Q, int64_t pstride, int64_t n, int64_t estride,
                                                                   double* __restrict__ wet, double* __restrict__ hyd, int axes_in_lds) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const double* s_y = c.axes;                       // very long axes stay in global memory (L1 / L2 hits)
    if (axes_in_lds) {
        double* t = reinterpret_cast<double*>(smem_raw);
        for (int i = threadIdx.x; i < c.ny + c.nx + c.nz; i += blockDim.x) t[i] = c.axes[i];
        __syncthreads();
        s_y = t;
    }
    const double* s_x = s_y + c.ny;
    const double* s_z = s_x + c.nx;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        double y, x, z;
        Q.point(i, y, x, z);
        double sw[E], sh[E];
        // out of bounds -> fill_value nan; nan coordinate -> nan (trilinear<>)
        const bool inside = (y >= c.y_lo) && (y <= c.y_hi) && (x >= c.x_lo) && (x <= c.x_hi) && (z >= c.z_lo) && (z <= c.z_hi);
        if (!inside) {
#pragma unroll
            for (int e = 0; e < E; ++e) { sw[e] = qnan(); sh[e] = qnan(); }
        } else {
            const int iy = find_cell(s_y, c.ny, y, c.y_lo, c.inv_dy, c.uni_y);
            const int ix = find_cell(s_x, c.nx, x, c.x_lo, c.inv_dx, c.uni_x);
            const int iz = find_cell(s_z, c.nz, z, c.z_lo, c.inv_dz, c.uni_z);
            const double ty = (y - s_y[iy]) / (s_y[iy + 1] - s_y[iy]);
            const double tx = (x - s_x[ix]) / (s_x[ix + 1] - s_x[ix]);
            const double tz = (z - s_z[iz]) / (s_z[iz + 1] - s_z[iz]);
            const int64_t o00 = ((int64_t)iy * c.nx + ix) * c.nz + iz;     // (y0,x0)
            const int64_t o01 = o00 + c.nz;                                // (y0,x1)
            const int64_t o10 = o00 + (int64_t)c.nx * c.nz;                // (y1,x0)
            const int64_t o11 = o10 + c.nz;                                // (y1,x1)
            const double wy0 = 1.0 - ty, wx0 = 1.0 - tx, wz0 = 1.0 - tz;
            const double a00 = wy0 * wx0, a01 = wy0 * tx, a10 = ty * wx0, a11 = ty * tx;
            const double k0 = a00 * wz0, k1 = a00 * tz, k2 = a01 * wz0, k3 = a01 * tz;
            const double k4 = a10 * wz0, k5 = a10 * tz, k6 = a11 * wz0, k7 = a11 * tz;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const T2* p = ev.v[e];
                double w[8], h[8];
                ld2(p + o00, w[0], h[0]); ld2(p + o00 + 1, w[1], h[1]);
                ld2(p + o01, w[2], h[2]); ld2(p + o01 + 1, w[3], h[3]);
                ld2(p + o10, w[4], h[4]); ld2(p + o10 + 1, w[5], h[5]);
                ld2(p + o11, w[6], h[6]); ld2(p + o11 + 1, w[7], h[7]);
                double aw = 0.0, ah = 0.0;
                aw += w[0] * k0; ah += h[0] * k0;
                aw += w[1] * k1; ah += h[1] * k1;
                aw += w[2] * k2; ah += h[2] * k2;
                aw += w[3] * k3; ah += h[3] * k3;
                aw += w[4] * k4; ah += h[4] * k4;
                aw += w[5] * k5; ah += h[5] * k5;
                aw += w[6] * k6; ah += h[6] * k6;
                aw += w[7] * k7; ah += h[7] * k7;
                sw[e] = aw; sh[e] = ah;
            }
        }
        // PointQuery::store's arithmetic (delay / divisor), the shared divisor made once
        const bool shared = pstride == 0;
        double up0 = 1.0;
        if (Q.pmode && shared) up0 = project_divisor(Q.pmode, Q.proj, Q.inc0, i);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            double w = sw[e], h = sh[e];
            if (Q.pmode) {
                const double up = shared ? up0 : project_divisor(Q.pmode, Q.proj + e * pstride, Q.inc0, i);
                w = w / up; h = h / up;
            }
            if (wet) wet[e * estride + i] = w;
            if (hyd) hyd[e * estride + i] = h;
        }
    }
}

}  // namespace rdr
