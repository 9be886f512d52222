// kiwi_linfit_wide.hpp -- the fit of kiwi_linfit.hpp for up to 64 basis sources per group, with an optional quadratic penalty
// and optional non-negative coefficients (multi-time-window slip inversion: kiwi_amd/slipfit.py).  Included by kiwi_hip.hip after
// kiwi_linfit.hpp, under the same -ffp-contract=off: every fp64 operation is rounded on its own, and
// tests/linfit_wide_restatement.py restates each in the same order (the GPU tests ask for bit identity).  Notation, layout
// (NN = K (K + 1) / 2 + K + 1: G upper triangle by rows, b, R), evaluation and chunk loop are kiwi_linfit.hpp's (linfit::run).
//   gram      K <= 8: linfit_gram_kernel<K>.  K > 8: linfit_wide_gram_kernel, one workgroup of 256 threads per (receiver, group,
//             pair of 8-wide basis tiles I <= J).  A thread keeps its tile's fp64 accumulators in registers: 64 for an
//             off-diagonal tile; 36 + the 8 b + R for a diagonal one (R is stored by tile (0, 0) alone).  Per time step it reads
//             the 16 (8) kept samples of its rows, and a diagonal tile d, once.  Rows past K of a ragged last tile are not read
//             (they accumulate zeros) and never stored.  EVERY element is summed in linfit_gram_kernel's order -- thread tid takes
//             samples tid, tid + 256, ... of the receiver's first slot, then of the next, into the same accumulator; wavefront tree
//             off = 32 .. 1; (w0 + w1) + (w2 + w3); times (double) dt -- so an element does not depend on K or on its tile, and
//             tests/linfit_restatement.py gram_by_receiver restates it for any K.  A row is read once per tile pair that holds it
//             (9 times for K = 64), from L2 / Infinity Cache after the first.  No atomics.
//   solve     linfit_wide_solve_kernel, one wavefront per group; the unscaled sums N, the scaled matrix A and the factor L are
//             triangles in LDS.  Fold: lanes over elements, receivers ascending, N[p] = N[p] + (w w) N_r[p] with the skip rules of
//             linfit_solve_kernel.  `normal` is N.  Penalty P (upper triangle by rows) if given: lam = 1, or, relative,
//             lam = (sum_i N_ii, ascending from zero) / K; Gp_ij = N_ij + lam P_ij.  A diagonal Gp_ii that is not positive: status 1,
//             pivot_min 0.  s_i = 1 / sqrt(Gp_ii); A_ij = (Gp_ji s_i) s_j for i > j, A_ii = 1; c_i = b_i s_i.
//             Cholesky over a passive set P (indices ascending; all of them when nonneg == 0), lanes over rows, each element by
//             the operation sequence of scaled_cholesky: column j: v_i = A_ij; v_i = v_i - L_ik L_jk (k < j in P ascending) for the
//             rows i >= j in P; pivot d = v_j, pivot test d > K 2^-52; L_jj = sqrt(d); L_ij = v_i / L_jj.  y_i = (c_i -
//             sum_{k < i} L_ik y_k) / L_ii; z_i = (y_i - sum_{k > i} L_ki z_k) / L_ii, i descending, k ascending.
//             nonneg == 0: x = z; a failed pivot is status 1 with the smallest pivot up to and including it; nsolves = 1.
//             nonneg == 1: a c_i or an A_ij that is not finite: status 1, pivot_min 0.  Otherwise
//             Lawson-Hanson on the normal equations, x = 0, P empty, no index barred, wave-uniform control flow:
//               1  w_i = c_i - sum_{j in P ascending} A_ij x_j for every i not in P and not barred; the largest, lowest index among
//                  equals (shuffles); none, or not > 10 K 2^-52 max_i |c_i|: finish.  Otherwise i* joins P.
//               2  3 K solves made: status 4, finish with the current (feasible) x.  Solve over P, count it.  A failed pivot: i*
//                  leaves P with x_i* = 0 and is barred for the rest of the call (a dependent column); go to 1.
//               3  every z_i > 0: x_P = z, go to 1.  Otherwise alpha = min over i in P with not z_i > 0 of x_i / (x_i - z_i) (0 where
//                  x_i - z_i is not positive), lowest index among equals; x_i = x_i + alpha (z_i - x_i) in P; the minimising index
//                  becomes exactly 0; every i in P with not x_i > 0 becomes 0 and leaves P; go to 2.
//             pivot_min is then the smallest pivot of the last solve that did not break down (1 if there was none).
//             coef_i = x_i s_i; misfit = sqrt(max((R - 2 x.b) + x.G.x, 0) / R) with the UNPENALISED sums, summed as
//             linfit_solve_kernel sums them; R not positive: status 1.  npositive counts x_i > 0.
// For K <= 8, nonneg == 0 and no penalty every output equals kiwi_hip_linear_fit's bit for bit.

namespace linfit {

constexpr int kWideTile = 8;                    // (kWideMaxBasis = 64 = one lane per row: kiwi_linfit.hpp)

// blockIdx.x = receiver, blockIdx.y = group, blockIdx.z = tile (DIAG) or pair of tiles I < J counted by rows (!DIAG)
template <bool DIAG>
__global__ __launch_bounds__(kThreads) void linfit_wide_gram_kernel(const float *__restrict__ proc, size_t syn_stride,
                                                                    const RecvDev *__restrict__ recv, const CompDev *__restrict__ comps,
                                                                    const float *__restrict__ reft, const float *__restrict__ reffilt,
                                                                    const FftPair *__restrict__ pairs, int nmis, int nrec, float syn_factor,
                                                                    float dt, int K, double *__restrict__ nbr)
{
    constexpr int T = kWideTile, NT = T * (T + 1) / 2;
    constexpr int NA = DIAG ? NT + T + 1 : T * T;
    __shared__ double part[kThreads / 64][NA];
    const int r = (int)blockIdx.x, g = (int)blockIdx.y, tid = (int)threadIdx.x;
    const RecvDev rd = recv[r];
    if (!rd.enabled) return;
    int I = (int)blockIdx.z, J = I;
    if (!DIAG) {
        const int nt = (K + T - 1) / T;
        int rem = I;
        I = 0;
        while (rem >= nt - 1 - I) { rem -= nt - 1 - I; I++; }
        J = I + 1 + rem;
    }
    const int na = min(T, K - I * T), nb = min(T, K - J * T);
    const int NG = K * (K + 1) / 2, NN = NG + K + 1;
    const bool unit = (syn_factor == 1.f);
    const float *__restrict__ srca = proc + ((size_t)g * K + (size_t)I * T) * syn_stride;
    const float *__restrict__ srcb = proc + ((size_t)g * K + (size_t)J * T) * syn_stride;
    double acc[NA];
#pragma unroll
    for (int p = 0; p < NA; p++) acc[p] = 0.0;
    for (int k = 0; k < rd.ncomp; k++) {
        const int slot = rd.slot0 + k;
        const CompDev cd = comps[slot];
        const size_t ofs = (size_t)cd.synofs + cd.halo;
        const float *__restrict__ dp = (cd.has_filter && pairs) ? reffilt + pairs[(size_t)g * K * nmis + slot].filtofs : reft + cd.refofs;
        for (int i = tid; i < cd.wlen; i += kThreads) {
            double sa[T];
#pragma unroll
            for (int a = 0; a < T; a++) {
                const float v = a < na ? srca[(size_t)a * syn_stride + ofs + i] : 0.f;
                sa[a] = (double)(unit ? v : syn_factor * v);
            }
            if (DIAG) {
                const double dv = (double)dp[i];
                int p = 0;
#pragma unroll
                for (int a = 0; a < T; a++)
#pragma unroll
                    for (int b = a; b < T; b++, p++) acc[p] = acc[p] + sa[a] * sa[b];
#pragma unroll
                for (int a = 0; a < T; a++) acc[NT + a] = acc[NT + a] + sa[a] * dv;
                acc[NA - 1] = acc[NA - 1] + dv * dv;
            } else {
                double sb[T];
#pragma unroll
                for (int b = 0; b < T; b++) {
                    const float v = b < nb ? srcb[(size_t)b * syn_stride + ofs + i] : 0.f;
                    sb[b] = (double)(unit ? v : syn_factor * v);
                }
#pragma unroll
                for (int a = 0; a < T; a++)
#pragma unroll
                    for (int b = 0; b < T; b++) acc[a * T + b] = acc[a * T + b] + sa[a] * sb[b];
            }
        }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int p = 0; p < NA; p++) {
        double v = acc[p];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v = v + __shfl_down(v, off, 64);
        if (lane == 0) part[wave][p] = v;
    }
    __syncthreads();
    if (tid < NA) {
        // where accumulator tid lives in the [NN] layout, if it is a row the tile has
        int p = -1;
        if (DIAG) {
            if (tid < NT) {
                int a = 0, rem = tid;
                while (rem >= T - a) { rem -= T - a; a++; }
                const int b = a + rem;
                if (b < na) p = tri(K, I * T + a, I * T + b);
            } else if (tid < NT + T) {
                if (tid - NT < na) p = NG + I * T + (tid - NT);
            } else if (I == 0) {
                p = NN - 1;
            }
        } else {
            const int a = tid / T, b = tid % T;
            if (a < na && b < nb) p = tri(K, I * T + a, J * T + b);
        }
        if (p >= 0) {
            const double t = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
            nbr[((size_t)g * nrec + r) * NN + p] = (double)dt * t;
        }
    }
}

__device__ __forceinline__ int wide_low(int i, int j) { return i * (i + 1) / 2 + j; }                   // j <= i
__device__ __forceinline__ bool wide_in(unsigned long long set, int i) { return (set >> i) & 1ull; }

// A_PP z = c_P over the passive set P (wave-uniform) by one wavefront, lane i = row i: false if a pivot failed.  z: lane i's z_i
// (0 outside P).  pmin: the smallest pivot up to and including the one that broke down.  tv: [kWideMaxBasis] scratch in LDS
__device__ __forceinline__ bool wide_cholesky(const double *A, double *L, const double *cv, double *tv, unsigned long long P, int K,
                                              double tol, int lane, double &z, double &pmin)
{
    const bool mine = lane < K && wide_in(P, lane);
    pmin = 1.0;
    z = 0.0;
    for (int j = 0; j < K; j++) {
        if (!wide_in(P, j)) continue;
        double v = 0.0;
        if (mine && lane >= j) {
            v = A[wide_low(lane, j)];
            for (int k = 0; k < j; k++)
                if (wide_in(P, k)) v = v - L[wide_low(lane, k)] * L[wide_low(j, k)];
        }
        const double d = __shfl(v, j, 64);
        if (d < pmin) pmin = d;
        if (!(d > tol)) return false;
        const double ljj = sqrt(d);
        if (mine && lane >= j) L[wide_low(lane, j)] = lane == j ? ljj : v / ljj;
        __syncthreads();
    }
    double v = mine ? cv[lane] : 0.0, y = 0.0;
    for (int j = 0; j < K; j++) {
        if (!wide_in(P, j)) continue;
        const double yj = __shfl(v, j, 64) / L[wide_low(j, j)];
        if (lane == j) y = yj;
        if (mine && lane > j) v = v - L[wide_low(lane, j)] * yj;
    }
    for (int i = K - 1; i >= 0; i--) {
        if (!wide_in(P, i)) continue;
        tv[lane] = (mine && lane > i) ? L[wide_low(lane, i)] * z : 0.0;
        __syncthreads();
        double t = __shfl(y, i, 64);
        for (int k = i + 1; k < K; k++)
            if (wide_in(P, k)) t = t - tv[k];
        const double zi = t / L[wide_low(i, i)];
        if (lane == i) z = zi;
        __syncthreads();
    }
    return true;
}

// w: [nrec] receiver weights with zeros for disabled receivers.  penalty: [K (K + 1) / 2] or null.  normal: [ng][NN] or null.
// One workgroup of one wavefront per group: every __syncthreads() below is reached by all 64 lanes (the control flow around
// them depends on wave-uniform values only).
__global__ __launch_bounds__(64) void linfit_wide_solve_kernel(const double *__restrict__ nbr, const double *__restrict__ w, int nrec,
                                                               int anarchy, int K, int nonneg, const double *__restrict__ penalty,
                                                               int relative, double *__restrict__ coef, double *__restrict__ misfit,
                                                               int *__restrict__ status, double *__restrict__ pivot_min,
                                                               int *__restrict__ npositive, int *__restrict__ nsolves,
                                                               double *__restrict__ normal)
{
    constexpr int KM = kWideMaxBasis, NGM = KM * (KM + 1) / 2;
    __shared__ double N[NGM + KM + 1], A[NGM], L[NGM], cv[KM], sv[KM], xv[KM], tv[KM];
    const int g = (int)blockIdx.x, lane = (int)threadIdx.x;
    const int NG = K * (K + 1) / 2, NN = NG + K + 1;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (int p = lane; p < NN; p += 64) N[p] = 0.0;
    for (int r = 0; r < nrec; r++) {
        double wr = w[r];
        if (wr == 0.0) continue;
        const double *__restrict__ q = nbr + ((size_t)g * nrec + r) * NN;
        if (anarchy) {
            const double Rr = q[NN - 1];
            wr = Rr > 0.0 ? wr / sqrt(Rr) : 0.0;
            if (wr == 0.0) continue;
        }
        const double w2 = wr * wr;
        for (int p = lane; p < NN; p += 64) N[p] = N[p] + w2 * q[p];
    }
    if (normal)
        for (int p = lane; p < NN; p += 64) normal[(size_t)g * NN + p] = N[p];
    __syncthreads();
    const double R = N[NN - 1];
    double lam = 1.0;
    if (penalty && relative) {
        lam = 0.0;
        for (int i = 0; i < K; i++) lam = lam + N[tri(K, i, i)];
        lam = lam / (double)K;
    }
    bool bad = false;
    if (lane < K) {
        double dii = N[tri(K, lane, lane)];
        if (penalty) dii = dii + lam * penalty[tri(K, lane, lane)];
        bad = !(dii > 0.0);
        const double s = 1.0 / sqrt(dii);
        sv[lane] = s;
        cv[lane] = N[NG + lane] * s;
        xv[lane] = 0.0;
    }
    const bool diag_ok = __ballot(bad) == 0ull;
    __syncthreads();
    int st = 0, nsol = 0;
    double pmin = 0.0, x = 0.0;                               // x: lane i's scaled x_i
    if (!diag_ok) {
        st = 1;
    } else {
        for (int i = 0; i < K; i++) {
            if (lane < i) {
                double gij = N[tri(K, lane, i)];
                if (penalty) gij = gij + lam * penalty[tri(K, lane, i)];
                A[wide_low(i, lane)] = (gij * sv[i]) * sv[lane];
            } else if (lane == i) {
                A[wide_low(i, i)] = 1.0;
            }
        }
        __syncthreads();
        // a non-finite gradient or step length would make the lanes of the active-set loop disagree: such a group has no solution
        bool wild = false;
        if (nonneg && lane < K) {
            wild = !isfinite(cv[lane]);
            for (int j = 0; j < lane; j++) wild = wild || !isfinite(A[wide_low(lane, j)]);
        }
        const bool finite = __ballot(wild) == 0ull;
        const double tol = (double)K * 2.220446049250313e-16;   // K 2^-52
        const unsigned long long all = K == 64 ? ~0ull : (1ull << K) - 1ull;
        if (!finite) {
            st = 1;
        } else if (!nonneg) {
            nsol = 1;
            double z;
            if (wide_cholesky(A, L, cv, tv, all, K, tol, lane, z, pmin)) x = z; else st = 1;
        } else {
            pmin = 1.0;
            double cmax = lane < K ? fabs(cv[lane]) : 0.0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) cmax = fmax(cmax, __shfl_xor(cmax, off, 64));
            const double thr = (10.0 * (double)K * 2.220446049250313e-16) * cmax;
            unsigned long long P = 0ull, barred = 0ull;
            for (;;) {
                // 1: the largest gradient component among the free indices
                const bool cand = lane < K && !wide_in(P | barred, lane);
                double bw = 0.0;
                if (cand) {
                    bw = cv[lane];
                    for (int j = 0; j < K; j++)
                        if (wide_in(P, j)) bw = bw - A[lane > j ? wide_low(lane, j) : wide_low(j, lane)] * xv[j];
                }
                int bi = cand ? lane : 64;                      // 64: no candidate
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    const double ow = __shfl_xor(bw, off, 64);
                    const int oi = __shfl_xor(bi, off, 64);
                    if (oi < 64 && (bi == 64 || ow > bw || (ow == bw && oi < bi))) { bw = ow; bi = oi; }
                }
                if (bi == 64 || !(bw > thr)) break;
                const int istar = bi;
                P |= 1ull << istar;
                bool again = true;
                while (again) {
                    // 2: solve over the passive set
                    if (nsol == 3 * K) { st = 4; break; }
                    nsol++;
                    double z, pm;
                    if (!wide_cholesky(A, L, cv, tv, P, K, tol, lane, z, pm)) {
                        P &= ~(1ull << istar);
                        barred |= 1ull << istar;
                        if (lane == istar) x = 0.0;
                        again = false;
                    } else {
                        pmin = pm;
                        const bool mine = lane < K && wide_in(P, lane);
                        const bool neg = mine && !(z > 0.0);
                        if (__ballot(neg) == 0ull) {
                            if (mine) x = z;
                            again = false;
                        } else {
                            // 3: the longest feasible step towards z
                            double al = 0.0;
                            if (neg) { const double den = x - z; al = den > 0.0 ? x / den : 0.0; }
                            int ai = neg ? lane : 64;
#pragma unroll
                            for (int off = 32; off > 0; off >>= 1) {
                                const double oa = __shfl_xor(al, off, 64);
                                const int oi = __shfl_xor(ai, off, 64);
                                if (oi < 64 && (ai == 64 || oa < al || (oa == al && oi < ai))) { al = oa; ai = oi; }
                            }
                            if (mine) x = x + al * (z - x);
                            if (lane == ai) x = 0.0;
                            const bool drop = mine && !(x > 0.0);
                            if (drop) x = 0.0;
                            P &= ~__ballot(drop);
                        }
                    }
                    if (lane < K) xv[lane] = x;
                    __syncthreads();
                }
                if (st != 0) break;
            }
        }
    }
    if (!(R > 0.0)) st = 1;
    // the data misfit of the coefficients, with the unpenalised sums
    const bool solved = st == 0 || st == 4;
    __syncthreads();
    const double cf = lane < K ? x * sv[lane] : 0.0;
    if (lane < K) xv[lane] = cf;
    __syncthreads();
    double mf = nan;
    if (solved) {
        double xb = 0.0;
        for (int i = 0; i < K; i++) xb = xb + xv[i] * N[NG + i];
        double row = 0.0;
        if (lane < K)
            for (int j = 0; j < K; j++) row = row + N[lane <= j ? tri(K, lane, j) : tri(K, j, lane)] * xv[j];
        tv[lane] = cf * row;
        __syncthreads();
        double xgx = 0.0;
        for (int i = 0; i < K; i++) xgx = xgx + tv[i];
        double val = (R - 2.0 * xb) + xgx;
        val = val > 0.0 ? val : 0.0;
        mf = sqrt(val / R);
    }
    const unsigned long long pos = __ballot(solved && lane < K && x > 0.0);
    if (lane < K) coef[(size_t)g * K + lane] = solved ? cf : nan;
    if (lane == 0) {
        misfit[g] = mf;
        status[g] = st;
        pivot_min[g] = pmin;
        npositive[g] = __popcll(pos);
        nsolves[g] = nsol;
    }
}

static void wide_launch(kiwi_hip_ctx *c, int K, int ng, const FftPair *pairs, const double *w_d, int anarchy, const Wide &wd,
                        const double *penalty_d, double *nbr, double *coef, double *misfit, int *status, double *pivot, int *npos,
                        int *nsol, double *normal, hipEvent_t between)
{
    const int nrec = (int)c->recv.size();
    if (K <= kMaxBasis) {
        launch_gram_any(c, K, ng, pairs, nbr);
    } else {
        const int nt = (K + kWideTile - 1) / kWideTile;
        hipLaunchKernelGGL(linfit_wide_gram_kernel<true>, dim3((unsigned)nrec, (unsigned)ng, (unsigned)nt), dim3(kThreads), 0, c->stream,
                           c->proc_d.p, c->syn_stride, c->recv_d.p, c->comps_d.p, c->reft_d.p, c->reffilt_d.p, pairs, c->nmis, nrec,
                           c->syn_factor, c->gm.dt, K, nbr);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(linfit_wide_gram_kernel<false>, dim3((unsigned)nrec, (unsigned)ng, (unsigned)(nt * (nt - 1) / 2)),
                           dim3(kThreads), 0, c->stream, c->proc_d.p, c->syn_stride, c->recv_d.p, c->comps_d.p, c->reft_d.p,
                           c->reffilt_d.p, pairs, c->nmis, nrec, c->syn_factor, c->gm.dt, K, nbr);
        HIPCHECK(hipGetLastError());
    }
    HIPCHECK(hipEventRecord(between, c->stream));
    hipLaunchKernelGGL(linfit_wide_solve_kernel, dim3((unsigned)ng), dim3(64), 0, c->stream, nbr, w_d, nrec, anarchy, K, wd.nonneg,
                       penalty_d, wd.relative, coef, misfit, status, pivot, npos, nsol, normal);
    HIPCHECK(hipGetLastError());
}

} // namespace linfit
