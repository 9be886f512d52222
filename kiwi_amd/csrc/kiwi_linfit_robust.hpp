// kiwi_linfit_robust.hpp -- the coefficients of kiwi_linfit.hpp under an l1 OUTER norm, by iteratively reweighted least squares
// (IRLS) on the device.  Included by kiwi_hip.hip right after kiwi_linfit.hpp, under the same -ffp-contract=off: every fp64
// operation below is rounded on its own, and tests/linfit_robust_restatement.py restates each in the same order (the GPU tests
// ask for bit identity).  Notation as in kiwi_linfit.hpp: s_k[t] the fp32 value the comparator compares of basis source k, d[t]
// the reference side, N_r = (G_r, b_r, R_r) the receiver's normal equations from linfit_gram_kernel, w_r = receiver_weight[r]
// (0 for a disabled receiver), T_r the total length of the windows of receiver r's slots.  A receiver with w_r == 0 or not
// R_r > 0 is skipped everywhere.  x_0 is what linfit_solve_kernel left in `coef` (same weights, same anarchy); a group it gave
// status 1 stays at status 1 and NaN.  Iterations i = 0 .. niter, all queued on the stream without a host round trip:
//
// Mode A (inner l1norm, outer l1norm): per iteration one launch of robust_pass_kernel and one of robust_step_kernel.
//   pass      one workgroup of 256 threads per (group, receiver), the sample order, accumulator sharing between slots and tree of
//             linfit_gram_kernel.  a_r = eps * sqrt(R_r / ((double) dt * (double) T_r)).  Per sample, with x the group's current
//             coefficients read from device memory:
//                 p = 0; p = p + x_k s_k[t] (k ascending); e = d[t] - p; ae = |e|; om = 1 / (ae > a_r ? ae : a_r); o_i = om s_i[t]
//             into NA = K (K + 1) / 2 + K + 3 fp64 accumulators per thread, in this order: G[i][j] (i <= j, by rows), b[i], L, H, D:
//                 G[i][j] += o_i s_j[t]    b[i] += o_i d[t]    L += ae    H += ae >= a_r ? ae - 0.5 a_r : (e e) / (2 a_r)    D += |d[t]|
//             the totals times (double) dt.  Each sample of each kept trace is read from memory once per pass.  No atomics.
//   step      one thread per group.  Receivers r ascending: v = w_r; anarchy: v = D_r > 0 ? w_r / D_r : 0, skipped if 0 (the
//             weights enter linearly: make_global_misfits' l1 branch); S[p] = S[p] + v S_r[p] for all NA sums.  Record
//             trace[i] = (S.H / S.D, S.L / S.D) and misfit = S.L / S.D.  For i < niter solve (S.G, S.b) by scaled_cholesky -- the
//             diagonal scaling, Cholesky and pivot test K 2^-52 of linfit_solve_kernel -- into the group's coefficients.
// Mode B (inner l2norm, outer l1norm): one launch of robust_receiver_kernel runs all iterations, one thread per group, on the
//   N_r alone.  Per iteration, receivers r ascending, x.b_r and x.G_r.x summed as linfit_solve_kernel sums them for its misfit:
//                 q = (R_r - 2 x.b_r) + x.G_r.x, clipped at 0; m = sqrt(q); n = sqrt(R_r); v = w_r, anarchy: v = w_r / n;
//                 a = eps n; u = v / (m > a ? m : a); S.G, S.b: S[p] = S[p] + u N_r[p];
//                 L = L + v m; H = H + v (m >= a ? m - 0.5 a : (m m) / (2 a)); D = D + v n
//   trace[i] = (H / D, L / D), misfit = L / D, then the same solve.
// Both: a solve that fails (a diagonal element not positive or a pivot <= K 2^-52) at iteration i sets status 3, leaves the
// coefficients x_i and their misfit and NaN in the later trace rows.  Groups with status != 0 before the first iteration have
// NaN trace rows throughout.

namespace linfit {

__device__ __forceinline__ double huber(double m, double a) { return m >= a ? m - 0.5 * a : (m * m) / (2.0 * a); }

// wbr: [group of the chunk][receiver][NA]; entries of skipped (group, receiver) pairs are neither written nor read
template <int K>
__global__ __launch_bounds__(kThreads) void robust_pass_kernel(const float *__restrict__ proc, size_t syn_stride,
                                                               const RecvDev *__restrict__ recv, const CompDev *__restrict__ comps,
                                                               const float *__restrict__ reft, const float *__restrict__ reffilt,
                                                               const FftPair *__restrict__ pairs, int nmis, int nrec, float syn_factor,
                                                               float dt, const double *__restrict__ nbr, const double *__restrict__ w,
                                                               const double *__restrict__ x, const int *__restrict__ status, double eps,
                                                               double *__restrict__ wbr)
{
    constexpr int NG = K * (K + 1) / 2, NN = NG + K + 1, NA = NG + K + 3;
    __shared__ double part[kThreads / 64][NA];
    const int r = (int)blockIdx.x, g = (int)blockIdx.y, tid = (int)threadIdx.x;
    if (status[g] != 0) return;
    const RecvDev rd = recv[r];
    if (!rd.enabled || w[r] == 0.0) return;
    const double Rr = nbr[((size_t)g * nrec + r) * NN + NN - 1];
    if (!(Rr > 0.0)) return;
    int T = 0;
    for (int k = 0; k < rd.ncomp; k++) T += comps[rd.slot0 + k].wlen;
    const double ar = eps * sqrt(Rr / ((double)dt * (double)T));
    double xs[K];
#pragma unroll
    for (int a = 0; a < K; a++) xs[a] = x[(size_t)g * K + a];
    const bool unit = (syn_factor == 1.f);
    const float *__restrict__ src0 = proc + (size_t)g * K * syn_stride;
    double acc[NA];
#pragma unroll
    for (int p = 0; p < NA; p++) acc[p] = 0.0;
    for (int k = 0; k < rd.ncomp; k++) {
        const int slot = rd.slot0 + k;
        const CompDev cd = comps[slot];
        const float *__restrict__ sy = src0 + cd.synofs + cd.halo;
        const float *__restrict__ dp = (cd.has_filter && pairs) ? reffilt + pairs[(size_t)g * K * nmis + slot].filtofs : reft + cd.refofs;
        for (int i = tid; i < cd.wlen; i += kThreads) {
            double s[K], o[K];
#pragma unroll
            for (int a = 0; a < K; a++) {
                const float v = sy[(size_t)a * syn_stride + i];
                s[a] = (double)(unit ? v : syn_factor * v);
            }
            const double dv = (double)dp[i];
            double pred = 0.0;
#pragma unroll
            for (int a = 0; a < K; a++) pred = pred + xs[a] * s[a];
            const double e = dv - pred, ae = fabs(e);
            const double om = 1.0 / (ae > ar ? ae : ar);
#pragma unroll
            for (int a = 0; a < K; a++) o[a] = om * s[a];
            int p = 0;
#pragma unroll
            for (int a = 0; a < K; a++)
#pragma unroll
                for (int b = a; b < K; b++, p++) acc[p] = acc[p] + o[a] * s[b];
#pragma unroll
            for (int a = 0; a < K; a++) acc[NG + a] = acc[NG + a] + o[a] * dv;
            acc[NG + K] = acc[NG + K] + ae;
            acc[NG + K + 1] = acc[NG + K + 1] + huber(ae, ar);
            acc[NG + K + 2] = acc[NG + K + 2] + fabs(dv);
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
        const double t = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
        wbr[((size_t)g * nrec + r) * NA + tid] = (double)dt * t;
    }
}

// iteration `it` of mode A for every group of the chunk: fold, record, and for it < niter solve into x
template <int K>
__global__ __launch_bounds__(64) void robust_step_kernel(const double *__restrict__ wbr, const double *__restrict__ nbr,
                                                         const double *__restrict__ w, int nrec, int anarchy, int ng, int it, int niter,
                                                         double *__restrict__ x, double *__restrict__ misfit, int *__restrict__ status,
                                                         double *__restrict__ trace)
{
    constexpr int NG = K * (K + 1) / 2, NN = NG + K + 1, NA = NG + K + 3;
    const int g = (int)(blockIdx.x * 64 + threadIdx.x);
    if (g >= ng) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double *__restrict__ tr = trace + ((size_t)g * (niter + 1) + it) * 2;
    if (status[g] != 0) { tr[0] = nan; tr[1] = nan; return; }
    double S[NA];
#pragma unroll
    for (int p = 0; p < NA; p++) S[p] = 0.0;
    for (int r = 0; r < nrec; r++) {
        const double wr = w[r];
        if (wr == 0.0 || !(nbr[((size_t)g * nrec + r) * NN + NN - 1] > 0.0)) continue;
        const double *__restrict__ q = wbr + ((size_t)g * nrec + r) * NA;
        double v = wr;
        if (anarchy) {
            const double Dr = q[NA - 1];
            v = Dr > 0.0 ? wr / Dr : 0.0;
            if (v == 0.0) continue;
        }
#pragma unroll
        for (int p = 0; p < NA; p++) S[p] = S[p] + v * q[p];
    }
    const double mis = S[NG + K] / S[NA - 1];
    tr[0] = S[NG + K + 1] / S[NA - 1];
    tr[1] = mis;
    misfit[g] = mis;
    if (it == niter) return;
    double xn[K], pmin;
    if (scaled_cholesky<K>(S, xn, pmin) != 0) { status[g] = 3; return; }
#pragma unroll
    for (int i = 0; i < K; i++) x[(size_t)g * K + i] = xn[i];
}

// mode B, all iterations of every group of the chunk
template <int K>
__global__ __launch_bounds__(64) void robust_receiver_kernel(const double *__restrict__ nbr, const double *__restrict__ w, int nrec,
                                                             int anarchy, int ng, int niter, double eps, double *__restrict__ x,
                                                             double *__restrict__ misfit, int *__restrict__ status,
                                                             double *__restrict__ trace)
{
    constexpr int NG = K * (K + 1) / 2, NN = NG + K + 1;
    const int g = (int)(blockIdx.x * 64 + threadIdx.x);
    if (g >= ng) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double *__restrict__ tr = trace + (size_t)g * (niter + 1) * 2;
    int it = 0;
    if (status[g] == 0) {
        double xc[K];
#pragma unroll
        for (int i = 0; i < K; i++) xc[i] = x[(size_t)g * K + i];
        for (;; it++) {
            double S[NG + K];
#pragma unroll
            for (int p = 0; p < NG + K; p++) S[p] = 0.0;
            double Ls = 0.0, Hs = 0.0, Ds = 0.0;
            for (int r = 0; r < nrec; r++) {
                const double wr = w[r];
                if (wr == 0.0) continue;
                const double *__restrict__ q = nbr + ((size_t)g * nrec + r) * NN;
                const double Rr = q[NN - 1];
                if (!(Rr > 0.0)) continue;
                double xb = 0.0, xgx = 0.0;
#pragma unroll
                for (int i = 0; i < K; i++) xb = xb + xc[i] * q[NG + i];
#pragma unroll
                for (int i = 0; i < K; i++) {
                    double row = 0.0;
#pragma unroll
                    for (int j = 0; j < K; j++) row = row + q[i <= j ? tri(K, i, j) : tri(K, j, i)] * xc[j];
                    xgx = xgx + xc[i] * row;
                }
                double val = (Rr - 2.0 * xb) + xgx;
                val = val > 0.0 ? val : 0.0;
                const double m = sqrt(val), n = sqrt(Rr);
                const double v = anarchy ? wr / n : wr;
                const double a = eps * n;
                const double u = v / (m > a ? m : a);
#pragma unroll
                for (int p = 0; p < NG + K; p++) S[p] = S[p] + u * q[p];
                Ls = Ls + v * m;
                Hs = Hs + v * huber(m, a);
                Ds = Ds + v * n;
            }
            const double mis = Ls / Ds;
            tr[2 * it] = Hs / Ds;
            tr[2 * it + 1] = mis;
            misfit[g] = mis;
            if (it == niter) break;
            double xn[K], pmin;
            if (scaled_cholesky<K>(S, xn, pmin) != 0) { status[g] = 3; break; }
#pragma unroll
            for (int i = 0; i < K; i++) xc[i] = xn[i];
        }
#pragma unroll
        for (int i = 0; i < K; i++) x[(size_t)g * K + i] = xc[i];
        it++;
    }
    for (; it <= niter; it++) { tr[2 * it] = nan; tr[2 * it + 1] = nan; }
}

// the reweighting of one chunk behind launch<K>: nbr, x (= coef), misfit and status as the l2 kernels left them on the stream
template <int K>
static void robust_launch(kiwi_hip_ctx *c, int ng, const FftPair *pairs, const double *w_d, int anarchy, const double *nbr,
                          const Robust &rb, double *wbr, double *x, double *misfit, int *status, double *trace)
{
    const int nrec = (int)c->recv.size();
    const dim3 per_group((unsigned)((ng + 63) / 64));
    if (rb.mode == 2) {
        hipLaunchKernelGGL(robust_receiver_kernel<K>, per_group, dim3(64), 0, c->stream, nbr, w_d, nrec, anarchy, ng, rb.niter, rb.eps, x,
                           misfit, status, trace);
        HIPCHECK(hipGetLastError());
        return;
    }
    for (int it = 0; it <= rb.niter; it++) {
        hipLaunchKernelGGL(robust_pass_kernel<K>, dim3((unsigned)nrec, (unsigned)ng), dim3(kThreads), 0, c->stream, c->proc_d.p,
                           c->syn_stride, c->recv_d.p, c->comps_d.p, c->reft_d.p, c->reffilt_d.p, pairs, c->nmis, nrec, c->syn_factor,
                           c->gm.dt, nbr, w_d, x, status, rb.eps, wbr);
        HIPCHECK(hipGetLastError());
        hipLaunchKernelGGL(robust_step_kernel<K>, per_group, dim3(64), 0, c->stream, wbr, nbr, w_d, nrec, anarchy, ng, it, rb.niter, x, misfit,
                           status, trace);
        HIPCHECK(hipGetLastError());
    }
}

static void robust_launch_any(kiwi_hip_ctx *c, int K, int ng, const FftPair *pairs, const double *w_d, int anarchy, const double *nbr,
                              const Robust &rb, double *wbr, double *x, double *misfit, int *status, double *trace)
{
    by_basis(K, [&](auto k) { robust_launch<k.value>(c, ng, pairs, w_d, anarchy, nbr, rb, wbr, x, misfit, status, trace); });
}

} // namespace linfit
