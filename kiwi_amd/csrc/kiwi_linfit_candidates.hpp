// kiwi_linfit_candidates.hpp -- what the evaluations of GIVEN coefficient vectors share (kiwi_linfit_candidates_timescan.hpp, which
// also serves the plain kiwi_hip_linear_fit_candidates as its one-offset case and holds the specification of the passes;
// kiwi_linfit_candidates_floating.hpp; kiwi_spectral_candidates.hpp): the quadratic form of a row of sums, the total order of
// "best" -- a NaN misfit never wins, then the smaller value, then the LOWER candidate index -- and the refusals of the plain call.
// Included by kiwi_hip.hip after kiwi_linfit_wide.hpp, under the same -ffp-contract=off.

namespace linfit {

constexpr int kCandThreads = 256;                   // candidates per workgroup
constexpr int kCandStage = 64;                      // receivers per LDS stage: 64 x NN x 8 bytes = 22.5 KiB at K = 8

// xb = x.b and xgx = x.G.x of the row q, summed as linfit_solve_kernel sums them for its misfit
template <int K>
__device__ __forceinline__ void quad(const double *q, const double (&x)[K], double &xb, double &xgx)
{
    constexpr int NG = K * (K + 1) / 2;
    xb = 0.0; xgx = 0.0;
#pragma unroll
    for (int i = 0; i < K; i++) xb = xb + x[i] * q[NG + i];
#pragma unroll
    for (int i = 0; i < K; i++) {
        double row = 0.0;
#pragma unroll
        for (int j = 0; j < K; j++) row = row + q[i <= j ? tri(K, i, j) : tri(K, j, i)] * x[j];
        xgx = xgx + x[i] * row;
    }
}

// (v, i) becomes (v2, i2) where that is the better one; i < 0: none
__device__ __forceinline__ void take_better(double &v, int &i, double v2, int i2)
{
    if (i2 >= 0 && (i < 0 || v2 < v || (v2 == v && i2 < i))) { v = v2; i = i2; }
}

__device__ __forceinline__ void wave_best(double &v, int &i)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double v2 = __shfl_down(v, off, 64);
        const int i2 = __shfl_down(i, off, 64);
        take_better(v, i, v2, i2);
    }
}

// what the candidate evaluation cannot do is refused before anything runs
static void check_candidates(const Candidates &cd, int K)
{
    if (cd.ncand < 1) throw std::runtime_error("linear_fit_candidates: ncand = " + std::to_string(cd.ncand) + "; at least one candidate is needed");
    if (!cd.x || !cd.best_index || !cd.best_misfit || !cd.status)
        throw std::runtime_error("linear_fit_candidates: null candidates, best_index, best_misfit or status array");
    if (cd.outer_norm != 1 && cd.outer_norm != 2) throw std::runtime_error("linear_fit_candidates: outer_norm must be 1 (l1norm) or 2 (l2norm)");
    if (cd.free_scale != 0 && cd.free_scale != 1)
        throw std::runtime_error("linear_fit_candidates: free_scale = " + std::to_string(cd.free_scale) + " must be 0 or 1");
    if (cd.free_scale && cd.outer_norm == 1)
        throw std::runtime_error("linear_fit_candidates: free_scale needs the outer l2norm (under l1norm the best scale of a direction has no closed form)");
    if (cd.scale && !cd.free_scale) throw std::runtime_error("linear_fit_candidates: a scale array without free_scale");
    if (K >= 1 && K <= kMaxBasis)
        for (size_t p = 0; p < (size_t)cd.ncand * K; p++)
            if (!std::isfinite(cd.x[p]))
                throw std::runtime_error("linear_fit_candidates: entry " + std::to_string(p % K) + " of candidate " + std::to_string(p / K) + " is not finite");
}

// kiwi_hip_linear_fit_candidates_params piece by piece (PieceCall, kiwi_group_run.hpp): linfit::run with the candidates behind its
// l2 kernels; out: the free fit made on the way
static PieceCall candidates_piece_call(int K, const double *receiver_weight, int anarchy, const Out &out, const Candidates &cd)
{
    return PieceCall{ K,
        [=](kiwi_hip_ctx *c) { check_candidates(cd, K); check_setup(c, K, out); },
        [=](kiwi_hip_ctx *c, int s0, int n) {
            const int nrec = (int)c->recv.size();
            fill_failed(n / K, K, nrec, out.at(s0 / K, K, nrec));
            linfit_candidates_timescan::fill_failed((size_t)(n / K), 1, (size_t)nrec, linfit_candidates_timescan::plain(cd.at(s0 / K, nrec)));
        },
        [=](kiwi_hip_ctx *c, int s0, int n) {
            const int nrec = (int)c->recv.size();
            const Candidates mine = cd.at(s0 / K, nrec);
            run(c, 0, n / K, K, receiver_weight, anarchy, out.at(s0 / K, K, nrec), nullptr, nullptr, &mine);
        } };
}

} // namespace linfit
