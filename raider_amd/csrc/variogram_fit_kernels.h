// Exponential variogram models of raiderStats (cli/statsPlot.py _fit_vario with __exponential__, nugget=False, :661-713) as exact bounded
// minima: per row f of h[F][M], gamma[F][M] (NaN in either = column absent) the range a and sill b of  b (1 - exp(-h / a))  that minimise
// scipy's soft_l1 cost over the reference's box.  The contract is in include/raider_hip.h (rdr_variogram_fit) and DESIGN 5l;
// tests/variogram_fit_model.py restates it in NumPy.  Included by raider_hip.hip after seasonal_kernels.h.
//
// One wave owns one row; no workgroup barrier, no atomic.  Two instantiations of one kernel, told apart by the row's present columns n:
//   WIDE = false  n <= 64.  The present columns are compacted into LDS in column order.  Lanes are range candidates: 8 per lane, one after
//                 the other, in the 512-point scan, one per lane in a refinement round.  A lane computes e_i = 1 - exp(-h_i / a) once per
//                 candidate and keeps it for every bisection step in an LDS column E[i][lane] (consecutive lanes, consecutive words);
//                 h and gamma are LDS broadcasts.  A lane adds its sums over i in column order.
//   WIDE = true   n > 64 (the binned=True total fit, up to D x nbins columns).  Lanes stride over the row's M columns in global memory,
//                 candidates run one after the other, e_i is recomputed in every bisection step, a sum is the lanes' partial sums (each in
//                 ascending column order) folded by the xor butterfly 32, 16, .. 1.
// Both are deterministic; they may differ from each other in round-off.  The argmin over (cost, candidate index) is a wave reduction by
// shuffles.  Each launch covers every row; a wave whose row belongs to the other instantiation returns after counting n.
#pragma once

constexpr int VF_FINE = 64;                   // candidates of a refinement round
constexpr int VF_ROUNDS = 8;                  // refinement rounds: the bracket shrinks by 2 / 63 in each
constexpr int VF_HALVINGS = 64;               // bisection steps at most (52 reach 2^-52 ub_b)
constexpr double VF_FLOOR_DIV = 38.0;         // exp(-38) < 2^-54: below h_pos / 38 every e of a positive lag is exactly 1
constexpr double VF_NEAR = 0x1p-40;           // "at" a bound of the range: within 2^-40 of it
enum { VF_AT_FLOOR = 1, VF_AT_UB_A = 2, VF_SILL_ZERO = 4, VF_SILL_UB = 8 };

struct VarioFitArgs {
    const double* h; const double* gamma; const double* ub;          // ub: NULL or [F][3]
    long long nfits; int m, k_scan;
    double f_scale;
    double* params; double* cost; double* rmse; long long* n; int* status; int* flags;
};

// what a lane needs to evaluate the objective at its candidate
struct VfRow {
    const double* h; const double* g;         // WIDE: the row in global memory [m]; else the compacted columns in LDS [n]
    double* E;                                // LDS [n][64] (not WIDE)
    int n;                                    // WIDE: m; else the present columns
    int lane;
    double inv_s, s2;
};

__device__ __forceinline__ double vf_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return __shfl(v, 0, 64);
}

// e of every present column at range a, kept for the bisection (not WIDE)
template <bool WIDE>
__device__ __forceinline__ void vf_prepare(const VfRow& R, double a) {
    if constexpr (!WIDE)
        for (int i = 0; i < R.n; ++i) R.E[i * 64 + R.lane] = 1.0 - exp(-R.h[i] / a);
}

// D(b) = sum e r / sqrt(1 + z)
template <bool WIDE>
__device__ __forceinline__ double vf_slope(const VfRow& R, double a, double b) {
    double acc = 0.0;
    if constexpr (WIDE) {
        for (int i = R.lane; i < R.n; i += 64) {
            const double h = R.h[i], g = R.g[i];
            if (h == h && g == g) {
                const double e = 1.0 - exp(-h / a), r = b * e - g, t = r * R.inv_s;
                acc += e * r / sqrt(1.0 + t * t);
            }
        }
        return vf_wave_sum(acc);
    } else {
        for (int i = 0; i < R.n; ++i) {
            const double e = R.E[i * 64 + R.lane], r = b * e - R.g[i], t = r * R.inv_s;
            acc += e * r / sqrt(1.0 + t * t);
        }
        return acc;
    }
}

// C = s^2 sum z / (sqrt(1 + z) + 1), and sum r^2
template <bool WIDE>
__device__ __forceinline__ double vf_cost(const VfRow& R, double a, double b, double* rr) {
    double acc = 0.0, sq = 0.0;
    if constexpr (WIDE) {
        for (int i = R.lane; i < R.n; i += 64) {
            const double h = R.h[i], g = R.g[i];
            if (h == h && g == g) {
                const double e = 1.0 - exp(-h / a), r = b * e - g, t = r * R.inv_s, z = t * t;
                acc += z / (sqrt(1.0 + z) + 1.0); sq += r * r;
            }
        }
        acc = vf_wave_sum(acc); sq = vf_wave_sum(sq);
    } else {
        for (int i = 0; i < R.n; ++i) {
            const double e = R.E[i * 64 + R.lane], r = b * e - R.g[i], t = r * R.inv_s, z = t * t;
            acc += z / (sqrt(1.0 + z) + 1.0); sq += r * r;
        }
    }
    *rr = sq;
    return R.s2 * acc;
}

// the sill of least cost in [0, ub_b] at range a (vf_prepare done): C is convex in b, D non-decreasing
template <bool WIDE>
__device__ __forceinline__ double vf_sill(const VfRow& R, double a, double ub_b, int* at) {
    *at = 0;
    if (vf_slope<WIDE>(R, a, 0.0) >= 0.0) { *at = VF_SILL_ZERO; return 0.0; }
    if (vf_slope<WIDE>(R, a, ub_b) <= 0.0) { *at = VF_SILL_UB; return ub_b; }
    double lo = 0.0, hi = ub_b;
    const double tol = 0x1p-52 * ub_b;
    for (int it = 0; it < VF_HALVINGS && hi - lo > tol; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (vf_slope<WIDE>(R, a, mid) > 0.0) hi = mid; else lo = mid;
    }
    return 0.5 * (lo + hi);
}

struct VfBest { double c, a, b, rr; int k, at; };

__device__ __forceinline__ double vf_candidate(double lo, double hi, double step, int k, int count) {
    return k == 0 ? lo : (k == count - 1 ? hi : lo * exp((double)k * step));
}

// `count` candidates spaced geometrically over [lo, hi] (a multiple of 64, or hi alone when lo >= hi): the one of least cost, each at its
// own best sill, the lowest index on ties - the same in every lane
template <bool WIDE>
__device__ __forceinline__ VfBest vf_round(const VfRow& R, double lo, double hi, double step, int count, double ub_b) {
    VfBest B; B.c = __longlong_as_double(0x7ff0000000000000ll); B.k = 0x7fffffff; B.a = hi; B.b = 0.0; B.rr = 0.0; B.at = 0;
    for (int k = WIDE ? 0 : R.lane; k < count; k += WIDE ? 1 : 64) {
        const double a = vf_candidate(lo, hi, step, k, count);
        vf_prepare<WIDE>(R, a);
        int at; double rr;
        const double b = vf_sill<WIDE>(R, a, ub_b, &at);
        double c = vf_cost<WIDE>(R, a, b, &rr);
        if (!(c == c)) c = __longlong_as_double(0x7ff0000000000000ll);
        if (c < B.c || (c == B.c && k < B.k)) { B.c = c; B.k = k; B.a = a; B.b = b; B.rr = rr; B.at = at; }
    }
    if constexpr (!WIDE) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            VfBest O;
            O.c = __shfl_xor(B.c, off, 64); O.a = __shfl_xor(B.a, off, 64); O.b = __shfl_xor(B.b, off, 64); O.rr = __shfl_xor(B.rr, off, 64);
            O.k = __shfl_xor(B.k, off, 64); O.at = __shfl_xor(B.at, off, 64);
            if (O.c < B.c || (O.c == B.c && O.k < B.k)) B = O;
        }
    }
    return B;
}

template <bool WIDE>
__global__ __launch_bounds__(64) void variogram_fit_kernel(VarioFitArgs A) {
    extern __shared__ double vf_lds[];        // not WIDE: h [64], gamma [64], E [min(m, 64)][64]
    const long long row = blockIdx.x;
    const int lane = threadIdx.x, m = A.m;
    const double* hr = A.h + (size_t)row * m;
    const double* gr = A.gamma + (size_t)row * m;
    const double inf = __longlong_as_double(0x7ff0000000000000ll), qnan = __longlong_as_double(0x7ff8000000000000ll);

    // the row: its present columns, the largest lag and value, the smallest positive lag, anything unusable
    int n = 0;
    double hmax = -inf, gmax = -inf, hpos = inf; bool bad = false;
    for (int base = 0; base < m; base += 64) {
        const int i = base + lane;
        double h = qnan, g = qnan;
        if (i < m) { h = hr[i]; g = gr[i]; }
        const bool present = h == h && g == g;
        const unsigned long long mask = __ballot(present);
        if (present) {
            hmax = h > hmax ? h : hmax; gmax = g > gmax ? g : gmax;
            if (h > 0.0 && h < hpos) hpos = h;
            if (h < 0.0 || h == inf || g == inf || g == -inf) bad = true;
            if constexpr (!WIDE) {
                const int pos = n + __popcll(mask & ((1ull << lane) - 1ull));
                if (pos < 64) { vf_lds[pos] = h; vf_lds[64 + pos] = g; }
            }
        }
        n += __popcll(mask);
    }
    if ((n > 64) != WIDE) return;             // the other instantiation's row (the whole wave leaves)
    __syncthreads();                          // one wave: orders the compacted columns before the lanes read each other's
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double a = __shfl_xor(hmax, off, 64), b = __shfl_xor(gmax, off, 64), c = __shfl_xor(hpos, off, 64);
        hmax = a > hmax ? a : hmax; gmax = b > gmax ? b : gmax; hpos = c < hpos ? c : hpos;
    }
    bad = __ballot(bad) != 0ull;

    double ub_a = 0.8 * hmax, ub_b = 0.8 * gmax, ub_c = 0.8 * gmax;
    if (A.ub) { ub_a = A.ub[row * 3]; ub_b = A.ub[row * 3 + 1]; ub_c = A.ub[row * 3 + 2]; }
    int status = 0;
    if (n == 0) status = 1;
    else if (bad) status = 2;
    else if (!(hpos < inf)) status = 3;
    else if (!(ub_a > 0.0 && ub_a < inf && ub_b > 0.0 && ub_b < inf)) status = 2;
    if (status != 0) {
        if (lane == 0) {
            A.params[row * 3] = qnan; A.params[row * 3 + 1] = qnan; A.params[row * 3 + 2] = qnan;
            A.cost[row] = qnan; A.rmse[row] = qnan; A.n[row] = n; A.status[row] = status; A.flags[row] = 0;
        }
        return;
    }

    VfRow R;
    R.h = WIDE ? hr : vf_lds; R.g = WIDE ? gr : vf_lds + 64; R.E = vf_lds + 128; R.n = WIDE ? m : n; R.lane = lane;
    R.inv_s = 1.0 / A.f_scale; R.s2 = A.f_scale * A.f_scale;

    const double a_floor = hpos / VF_FLOOR_DIV;
    double lo = a_floor, hi = ub_a;
    int count = A.k_scan;
    const bool single = !(ub_a > a_floor);    // the whole box lies on the plateau: one candidate, ub_a
    if (single) { lo = ub_a; count = 64; }
    double step = single ? 0.0 : log(hi / lo) / (double)(count - 1);
    VfBest G = vf_round<WIDE>(R, lo, hi, step, count, ub_b);
    if (!single) {
        VfBest B = G;
        for (int r = 0; r < VF_ROUNDS; ++r) {
            const int k0 = B.k > 0 ? B.k - 1 : 0, k1 = B.k < count - 1 ? B.k + 1 : count - 1;
            const double nlo = vf_candidate(lo, hi, step, k0, count), nhi = vf_candidate(lo, hi, step, k1, count);
            lo = nlo; hi = nhi; count = VF_FINE;
            step = log(hi / lo) / (double)(count - 1);
            B = vf_round<WIDE>(R, lo, hi, step, count, ub_b);
            if (B.c < G.c) G = B;             // (a tie stays with the earlier round)
        }
    }
    if (lane == 0) {
        int flags = G.at;
        if (G.a <= a_floor + VF_NEAR * a_floor) flags |= VF_AT_FLOOR;
        if (G.a >= ub_a - VF_NEAR * ub_a) flags |= VF_AT_UB_A;
        A.params[row * 3] = G.a; A.params[row * 3 + 1] = G.b; A.params[row * 3 + 2] = 0.5 * ub_c;
        A.cost[row] = G.c; A.rmse[row] = sqrt(G.rr / (double)n); A.n[row] = n; A.status[row] = 0; A.flags[row] = flags;
    }
}
