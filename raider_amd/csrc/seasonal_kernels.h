// Seasonal sinusoids of raiderStats (cli/statsPlot.py _amplitude_and_phase, :2311-2479, and the grid_seasonal_* maps, :1796-2309): per
// station the exact linear least-squares fit of  y ~ a sin(w tau) + b cos(w tau) + c  to a [nd][n] series with NaN = no row, at one
// given angular frequency (fixed mode) or at the frequency of a band where the residual sum R(w) is smallest (scan mode).  Included by
// raider_hip.hip after grid_stats_kernels.h.  tau = t - t_ref, t_ref the middle of the date axis; y is taken relative to the station's
// mean.  Per (station, frequency) the sums over the station's dates that hold a value
//     n, S s, S c, S ss, S sc, S ys, S yc, S y, S yy           (S cc = n - S ss)
// give a, b, c and R in closed form (sf_solve).
//
// Five kernels, lanes over stations everywhere (a row of `values` is read by consecutive lanes, coalesced), every sum added by ONE lane
// in date order: the same bytes on every run, for host and device inputs, and for every split of the work.  No floating-point atomic.
//   seasonal_prep_kernel   n, mean, S y, S yy, the span of the station's rows and the eligibility rule of :2346-2347.
//   seasonal_table_kernel  sin and cos of w_k tau_d, once per (k, d): they are the same for every station.  Laid out [tile][d][SF_KT],
//                          so the SF_KT pairs a wave needs at one date are 128 contiguous bytes, read through the scalar cache.
//   seasonal_scan_kernel   a wave owns 64 stations and a segment of frequency tiles; per tile a register tile of SF_KT frequencies x 6
//                          sums per lane, a sequential walk over the dates; it keeps the lowest R of its segment (the lowest k on
//                          ties) and writes (R, k) per (segment, station).  The segments only spread the work: R(w_k) does not depend
//                          on them, and the fit kernel takes their minimum in ascending order.
//   seasonal_fit_kernel    k* = argmin over the segments; a golden-section search of R inside [w_(k*-1), w_(k*+1)] (clipped to the band)
//                          with sin / cos per lane, until the bracket is below 1e-10 of the grid step, the two inner values are equal
//                          (R is flat to round-off) or SF_MAXIT steps; the best frequency evaluated wins.  Then, at that frequency
//                          (fixed mode: at the given one), one pass for the analytic Jacobian of (A, [w,] p, c) and the outputs.
//   seasonal_cell_kernel   per grid cell and column the plain mean over the cell's fitted stations and the mean weighted by their row
//                          counts, added in station order.
#pragma once

constexpr int SF_KT = 8;                      // frequencies of a register tile: 6 x 8 = 48 f64 accumulators per lane
constexpr int SF_MAXIT = 64;                  // golden-section steps at most (0.618^64 of the bracket is far below 1e-10 of a grid step)
constexpr int SF_NCOL = 16;                   // rows of the station output
constexpr int SF_NREF = 7;                    // the reference's station columns (phsfit, ampfit, periodfit, phsfit_c, ampfit_c, periodfit_c, rmse)
constexpr double SF_YEAR = 31556952.0;        // the reference's seconds per year
enum { SF_NOBS = 0, SF_SPAN, SF_FITTED, SF_EDGE, SF_AMP, SF_PHASE, SF_OFFSET, SF_OMEGA, SF_RSS, SF_RMSE, SF_SIG_AMP, SF_SIG_OMEGA, SF_SIG_PHASE,
       SF_SIG_OFFSET, SF_KSTAR, SF_ITER };

struct SeasonalArgs {
    const double* tau; const double* values; const double* omega; const long long* cell_start;
    long long n; int nd, k, scan, ntiles, nseg, tiles_per_seg, ncells;
    double min_span, min_frac, t_ref;
    double2* table;                           // [ntiles][nd][SF_KT] (sin, cos)
    double* prep;                             // [5][n]: n, mean, S y, S yy, fitted
    double* best;                             // [nseg][2][n]: R, k
    double* station;                          // [SF_NCOL][n]
    double* cells;                            // [2 * SF_NREF][ncells]
};

struct SfFit { double a, b, c, R; };          // c relative to the station's mean

// the closed form: eliminate c, solve the 2 x 2 system of the centred sums.  R = NaN where the system is singular (det <= 0).
__device__ __forceinline__ SfFit sf_solve(double n, double s, double c, double ss, double sc, double ys, double yc, double sy, double syy) {
    const double cc = n - ss;
    const double Sss = ss - s * s / n, Ssc = sc - s * c / n, Scc = cc - c * c / n;
    const double Sys = ys - s * sy / n, Syc = yc - c * sy / n, Syy = syy - sy * sy / n;
    const double det = Sss * Scc - Ssc * Ssc;
    SfFit f;
    if (!(det > 0.0)) { f.a = f.b = f.c = f.R = __longlong_as_double(0x7ff8000000000000ll); return f; }
    f.a = (Sys * Scc - Syc * Ssc) / det;
    f.b = (Syc * Sss - Sys * Ssc) / det;
    f.c = (sy - f.a * s - f.b * c) / n;
    const double R = Syy - f.a * Sys - f.b * Syc;
    f.R = R > 0.0 ? R : 0.0;
    return f;
}

__global__ __launch_bounds__(64) void seasonal_prep_kernel(SeasonalArgs A) {
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    if (s >= A.n) return;
    const size_t n = (size_t)A.n;
    const double* col = A.values + s;
    double sum = 0.0, tmin = 0.0, tmax = 0.0; int m = 0;
    for (int d = 0; d < A.nd; ++d) {
        const double v = col[(size_t)d * n];
        if (v == v) {
            const double t = A.tau[d];
            if (m == 0 || t < tmin) tmin = t;
            if (m == 0 || t > tmax) tmax = t;
            sum += v; ++m;
        }
    }
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double mean = m ? sum / (double)m : qnan;
    double sy = 0.0, syy = 0.0;
    for (int d = 0; d < A.nd; ++d) {
        const double v = col[(size_t)d * n];
        if (v == v) { const double y = v - mean; sy += y; syy += y * y; }
    }
    const double span = m ? (tmax - tmin) / SF_YEAR : qnan;
    const int P = A.scan ? 4 : 3;
    const bool ok = m >= P + 1 && span >= A.min_span && (double)m / (span * 365.25) >= A.min_frac;
    A.prep[s] = (double)m; A.prep[n + s] = mean; A.prep[2 * n + s] = sy; A.prep[3 * n + s] = syy; A.prep[4 * n + s] = ok ? 1.0 : 0.0;
    A.station[(size_t)SF_NOBS * n + s] = (double)m;
    A.station[(size_t)SF_SPAN * n + s] = span;
}

__global__ __launch_bounds__(256) void seasonal_table_kernel(SeasonalArgs A) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long total = (long long)A.ntiles * A.nd * SF_KT;
    if (q >= total) return;
    const int j = (int)(q % SF_KT);
    const long long r = q / SF_KT;
    const int d = (int)(r % A.nd), tile = (int)(r / A.nd);
    int k = tile * SF_KT + j; k = k < A.k ? k : A.k - 1;          // (the padding of the last tile repeats the last frequency)
    double sn, cs;
    sincos(A.omega[k] * A.tau[d], &sn, &cs);
    A.table[q] = make_double2(sn, cs);
}

__global__ __launch_bounds__(64) void seasonal_scan_kernel(SeasonalArgs A) {
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    const size_t n = (size_t)A.n;
    const bool live = s < A.n && A.prep[4 * n + s] != 0.0;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    const double* col = A.values + (s < A.n ? s : 0);
    const int nd = A.nd, seg = blockIdx.y;
    const double m = live ? A.prep[s] : 0.0, mean = live ? A.prep[n + s] : 0.0, sy = live ? A.prep[2 * n + s] : 0.0, syy = live ? A.prep[3 * n + s] : 0.0;
    const int tile0 = seg * A.tiles_per_seg;
    int tile1 = tile0 + A.tiles_per_seg; tile1 = tile1 < A.ntiles ? tile1 : A.ntiles;
    double bestR = __longlong_as_double(0x7ff0000000000000ll), bestk = -1.0;
    for (int tile = tile0; tile < tile1; ++tile) {
        const double2* __restrict__ tab = A.table + (size_t)tile * nd * SF_KT;
        double as[SF_KT], ac[SF_KT], ass[SF_KT], asc[SF_KT], ays[SF_KT], ayc[SF_KT];
#pragma unroll
        for (int j = 0; j < SF_KT; ++j) as[j] = ac[j] = ass[j] = asc[j] = ays[j] = ayc[j] = 0.0;
        auto add = [&](double v, int d) {
            if (v == v) {
                const double y = v - mean;
#pragma unroll
                for (int j = 0; j < SF_KT; ++j) {
                    const double2 t = tab[(size_t)d * SF_KT + j];
                    as[j] += t.x; ac[j] += t.y; ass[j] += t.x * t.x; asc[j] += t.x * t.y; ays[j] += y * t.x; ayc[j] += y * t.y;
                }
            }
        };
        int d = 0;
        for (; d + 3 < nd; d += 4) {          // four loads in flight
            double v0 = qnan, v1 = qnan, v2 = qnan, v3 = qnan;
            if (live) { v0 = col[(size_t)d * n]; v1 = col[(size_t)(d + 1) * n]; v2 = col[(size_t)(d + 2) * n]; v3 = col[(size_t)(d + 3) * n]; }
            add(v0, d); add(v1, d + 1); add(v2, d + 2); add(v3, d + 3);
        }
        for (; d < nd; ++d) add(live ? col[(size_t)d * n] : qnan, d);
        if (live) {
#pragma unroll
            for (int j = 0; j < SF_KT; ++j) {
                const int k = tile * SF_KT + j;
                const SfFit f = sf_solve(m, as[j], ac[j], ass[j], asc[j], ays[j], ayc[j], sy, syy);
                if (k < A.k && f.R < bestR) { bestR = f.R; bestk = (double)k; }
            }
        }
    }
    if (s < A.n) {
        A.best[((size_t)seg * 2) * n + s] = bestR;
        A.best[((size_t)seg * 2 + 1) * n + s] = bestk;
    }
}

// the fit of one station's column at the angular frequency w, sin and cos computed by the lane, the dates in order
__device__ __forceinline__ SfFit sf_eval(const double* col, size_t n, int nd, const double* __restrict__ tau, double m, double mean, double sy, double syy,
                                          double w) {
    double as = 0.0, ac = 0.0, ass = 0.0, asc = 0.0, ays = 0.0, ayc = 0.0;
    for (int d = 0; d < nd; ++d) {
        const double v = col[(size_t)d * n];
        if (v == v) {
            const double y = v - mean;
            double sn, cs;
            sincos(w * tau[d], &sn, &cs);
            as += sn; ac += cs; ass += sn * sn; asc += sn * cs; ays += y * sn; ayc += y * cs;
        }
    }
    return sf_solve(m, as, ac, ass, asc, ays, ayc, sy, syy);
}

// the inverse of the symmetric positive definite P x P matrix M, through its unit-diagonal scaling and Gauss-Jordan steps without pivoting
template <int P>
__device__ __forceinline__ void sf_invert(double (&M)[P][P]) {
    double sc[P];
#pragma unroll
    for (int i = 0; i < P; ++i) sc[i] = 1.0 / sqrt(M[i][i]);
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) M[i][j] *= sc[i] * sc[j];
#pragma unroll
    for (int p = 0; p < P; ++p) {
        const double ip = 1.0 / M[p][p];
        M[p][p] = 1.0;
#pragma unroll
        for (int j = 0; j < P; ++j) M[p][j] *= ip;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            if (i == p) continue;
            const double f = M[i][p];
            M[i][p] = 0.0;
#pragma unroll
            for (int j = 0; j < P; ++j) M[i][j] -= f * M[p][j];
        }
    }
#pragma unroll
    for (int i = 0; i < P; ++i)
#pragma unroll
        for (int j = 0; j < P; ++j) M[i][j] *= sc[i] * sc[j];
}

__global__ __launch_bounds__(64) void seasonal_fit_kernel(SeasonalArgs A) {
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    if (s >= A.n) return;
    const size_t n = (size_t)A.n;
    const double qnan = __longlong_as_double(0x7ff8000000000000ll), inf = __longlong_as_double(0x7ff0000000000000ll);
    const double pi = 3.14159265358979323846, two_pi = 6.28318530717958647692;
    double* out = A.station + s;
    auto none = [&]() {
        for (int r = SF_FITTED; r < SF_NCOL; ++r) out[(size_t)r * n] = qnan;
        out[(size_t)SF_FITTED * n] = 0.0; out[(size_t)SF_EDGE * n] = 0.0;
    };
    if (A.prep[4 * n + s] == 0.0) { none(); return; }
    const double* col = A.values + s;
    const double* __restrict__ tau = A.tau;
    const int nd = A.nd;
    const double m = A.prep[s], mean = A.prep[n + s], sy = A.prep[2 * n + s], syy = A.prep[3 * n + s];

    double w = A.omega[0], kstar = 0.0, edge = 0.0; int iters = 0;
    SfFit fit;
    if (A.scan) {
        double bR = inf, bk = -1.0;
        for (int g = 0; g < A.nseg; ++g) {    // ascending k: the lowest index wins a tie
            const double R = A.best[((size_t)g * 2) * n + s];
            if (R < bR) { bR = R; bk = A.best[((size_t)g * 2 + 1) * n + s]; }
        }
        if (bk < 0.0) { none(); return; }     // singular at every frequency of the band
        const int ks = (int)bk;
        kstar = bk; edge = (ks == 0 || ks == A.k - 1) ? 1.0 : 0.0;
        w = A.omega[ks];
        fit = sf_eval(col, n, nd, tau, m, mean, sy, syy, w);
        double lo = A.omega[ks > 0 ? ks - 1 : 0], hi = A.omega[ks < A.k - 1 ? ks + 1 : A.k - 1];
        const double tol = A.k > 1 ? 1e-10 * (A.omega[1] - A.omega[0]) : 0.0;
        const double g = 0.6180339887498949;
        auto val = [&](const SfFit& f) { return f.R == f.R ? f.R : inf; };
        if (hi - lo >= tol && hi > lo) {
            double x1 = hi - g * (hi - lo), x2 = lo + g * (hi - lo);
            SfFit f1 = sf_eval(col, n, nd, tau, m, mean, sy, syy, x1), f2 = sf_eval(col, n, nd, tau, m, mean, sy, syy, x2);
            if (val(f1) < val(fit)) { fit = f1; w = x1; }
            if (val(f2) < val(fit)) { fit = f2; w = x2; }
            while (iters < SF_MAXIT && hi - lo >= tol && val(f1) != val(f2)) {
                ++iters;
                if (val(f1) < val(f2)) {
                    hi = x2; x2 = x1; f2 = f1; x1 = hi - g * (hi - lo);
                    f1 = sf_eval(col, n, nd, tau, m, mean, sy, syy, x1);
                    if (val(f1) < val(fit)) { fit = f1; w = x1; }
                } else {
                    lo = x1; x1 = x2; f1 = f2; x2 = lo + g * (hi - lo);
                    f2 = sf_eval(col, n, nd, tau, m, mean, sy, syy, x2);
                    if (val(f2) < val(fit)) { fit = f2; w = x2; }
                }
            }
        }
    } else {
        fit = sf_eval(col, n, nd, tau, m, mean, sy, syy, w);
    }
    if (!(fit.R == fit.R)) { none(); return; }

    // J^T J of (A, [w,] p, c) with tau centred and in years; u = sin(phi), v = A cos(phi), phi = w tau + p_c
    const double amp = hypot(fit.a, fit.b), pc = atan2(fit.b, fit.a);
    double Juu = 0.0, Juv = 0.0, Jvv = 0.0, Ju = 0.0, Jv = 0.0, Juw = 0.0, Jvw = 0.0, Jww = 0.0, Jw = 0.0;
    const double ia = 1.0 / amp;
    for (int d = 0; d < nd; ++d) {
        const double v0 = col[(size_t)d * n];
        if (v0 == v0) {
            double sn, cs;
            sincos(w * tau[d], &sn, &cs);
            const double u = (fit.a * sn + fit.b * cs) * ia, v = fit.a * cs - fit.b * sn, ty = tau[d] / SF_YEAR, ww = ty * v;
            Juu += u * u; Juv += u * v; Jvv += v * v; Ju += u; Jv += v;
            Juw += u * ww; Jvw += v * ww; Jww += ww * ww; Jw += ww;
        }
    }
    double sA, sW = qnan, sP, sC;
    if (A.scan) {
        const double s2 = fit.R / (m - 4.0);
        double M[4][4] = {{Juu, Juw, Juv, Ju}, {Juw, Jww, Jvw, Jw}, {Juv, Jvw, Jvv, Jv}, {Ju, Jw, Jv, m}};
        sf_invert<4>(M);
        const double ty = A.t_ref / SF_YEAR;                      // p = p_c - w t_ref
        sA = sqrt(s2 * M[0][0]); sW = sqrt(s2 * M[1][1]) / SF_YEAR;
        sP = sqrt(s2 * (M[2][2] - 2.0 * ty * M[1][2] + ty * ty * M[1][1]));
        sC = sqrt(s2 * M[3][3]);
    } else {
        const double s2 = fit.R / (m - 3.0);
        double M[3][3] = {{Juu, Juv, Ju}, {Juv, Jvv, Jv}, {Ju, Jv, m}};
        sf_invert<3>(M);
        sA = sqrt(s2 * M[0][0]); sP = sqrt(s2 * M[1][1]); sC = sqrt(s2 * M[2][2]);
    }
    double x = pc - w * A.t_ref;
    double p = x - two_pi * rint(x / two_pi);
    if (p <= -pi) p += two_pi;
    if (p > pi) p -= two_pi;
    const double rmse = sqrt(fit.R / (m - 2.0)), off = mean + fit.c;
    const bool fin = isfinite(amp) && isfinite(p) && isfinite(off) && isfinite(rmse) && isfinite(sA) && isfinite(sP) && isfinite(sC) && (!A.scan || isfinite(sW));
    if (!fin) { none(); return; }
    out[(size_t)SF_FITTED * n] = 1.0; out[(size_t)SF_EDGE * n] = edge;
    out[(size_t)SF_AMP * n] = amp; out[(size_t)SF_PHASE * n] = p; out[(size_t)SF_OFFSET * n] = off; out[(size_t)SF_OMEGA * n] = w;
    out[(size_t)SF_RSS * n] = fit.R; out[(size_t)SF_RMSE * n] = rmse;
    out[(size_t)SF_SIG_AMP * n] = sA; out[(size_t)SF_SIG_OMEGA * n] = sW; out[(size_t)SF_SIG_PHASE * n] = sP; out[(size_t)SF_SIG_OFFSET * n] = sC;
    out[(size_t)SF_KSTAR * n] = A.scan ? kstar : qnan; out[(size_t)SF_ITER * n] = (double)iters;
}

// the reference's column `c` of a fitted station: phsfit, ampfit, periodfit, phsfit_c, ampfit_c, periodfit_c, seasonalfit_rmse - with its
// labels: pcov[1, 1] is "periodfit_c" and pcov[2, 2] "phsfit_c", whatever the parameters are (:2424-2426)
__device__ __forceinline__ double sf_refcol(const double* st, size_t n, int c, int scan) {
    switch (c) {
        case 0: return (365.25 / 2.0) * sin(st[(size_t)SF_PHASE * n]);
        case 1: return st[(size_t)SF_AMP * n];
        case 2: return 1.0 / ((st[(size_t)SF_OMEGA * n] / 6.28318530717958647692) * SF_YEAR);
        case 3: return st[(size_t)(scan ? SF_SIG_PHASE : SF_SIG_OFFSET) * n];
        case 4: return st[(size_t)SF_SIG_AMP * n];
        case 5: return st[(size_t)(scan ? SF_SIG_OMEGA : SF_SIG_PHASE) * n];
        default: return st[(size_t)SF_RMSE * n];
    }
}

__global__ __launch_bounds__(256) void seasonal_cell_kernel(SeasonalArgs A) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= (long long)A.ncells * SF_NREF) return;
    const int cell = (int)(q / SF_NREF), c = (int)(q % SF_NREF);
    const size_t n = (size_t)A.n;
    double sum = 0.0, wsum = 0.0, cnt = 0.0, rows = 0.0;
    for (long long s = A.cell_start[cell]; s < A.cell_start[cell + 1]; ++s) {
        if (A.station[(size_t)SF_FITTED * n + s] != 0.0) {
            const double v = sf_refcol(A.station + s, n, c, A.scan), m = A.station[(size_t)SF_NOBS * n + s];
            sum += v; cnt += 1.0; wsum += m * v; rows += m;
        }
    }
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    A.cells[(size_t)c * A.ncells + cell] = cnt > 0.0 ? sum / cnt : qnan;
    A.cells[(size_t)(SF_NREF + c) * A.ncells + cell] = cnt > 0.0 ? wsum / rows : qnan;
}
