// nl_score.h -- scoring reduction over logits rows (nl_score, nl_op_score_rows): per row the log-sum-exp, the log-probability
// of a target id and the greedy id, in one pass over the row.  No reference counterpart in the Go engine; the quantity is the
// cross entropy nanollama/core_eval.py computes with torch (log-softmax of the row at the target).
#pragma once
#include "nl_kernels.h"

namespace nl {

// exp(x) in float64, the chain of exp_f64_as_f32 (nl_kernels.h) without the final rounding to float32: Cody-Waite reduction,
// degree-13 Taylor polynomial in Estrin form, v_ldexp_f64; <= 2 ulp.  The callers pass x <= 0; -inf and x < -745 give 0.
__device__ __forceinline__ double exp_f64_chain(double xin) {
    const double x = fmin(fmax(xin, -750.0), 710.0);
    const double k = rint(x * 1.44269504088896338700e+00);
    double r = fma(k, -6.93147180369123816490e-01, x);
    r = fma(k, -1.90821492927058770002e-10, r);
    const double r2 = r * r, r4 = r2 * r2, r8 = r4 * r4;
    const double a0 = 1.0 + r;
    const double a1 = fma(r, 1.0 / 6, 1.0 / 2), a2 = fma(r, 1.0 / 120, 1.0 / 24), a3 = fma(r, 1.0 / 5040, 1.0 / 720);
    const double a4 = fma(r, 1.0 / 362880, 1.0 / 40320), a5 = fma(r, 1.0 / 39916800, 1.0 / 3628800);
    const double a6 = fma(r, 1.0 / 6227020800.0, 1.0 / 479001600);
    const double b0 = fma(a1, r2, a0), b1 = fma(a3, r2, a2), b2 = fma(a5, r2, a4);
    const double d0 = fma(b1, r4, b0), d1 = fma(a6, r4, b2);
    return ldexp(fma(d1, r8, d0), (int)k);
}

// What a thread, a wavefront and the workgroup know of a row: the running maximum m, s = sum exp(x - m) over the entries seen
// (float64), and idx, the lowest index at which m stands (go/main.go:400-408: strict >, so the first of equals wins).
// m == -inf: nothing finite seen yet, s == 0.
struct ScoreAcc {
    float m;
    double s;
    int idx;
};
constexpr int SCORE_NO_IDX = 0x7fffffff;      // nothing seen: any index is lower

// exp(a - m) for a <= m, either possibly -inf: a == m gives exactly 1 (also for -inf == -inf, where a - m would be NaN)
__device__ __forceinline__ double score_scale(float a, float m) { return a == m ? 1.0 : exp_f64_chain((double)a - (double)m); }

// fold b into a; symmetric (both orders give the same bits: a float64 sum of two products and a max), so the butterfly
// below leaves every lane of a wavefront with the same value
__device__ __forceinline__ void score_merge(ScoreAcc &a, float bm, double bs, int bidx) {
    if (bm > a.m || (bm == a.m && bidx < a.idx)) a.idx = bidx;
    const float m = fmaxf(a.m, bm);
    const double ta = a.s * score_scale(a.m, m), tb = bs * score_scale(bm, m);
    a.s = ta + tb;
    a.m = m;
}

template <int CTRL>
__device__ __forceinline__ void score_merge_dpp(ScoreAcc &a) {
    const float bm = dpp_f32<CTRL>(a.m);
    const double bs = dpp_f64<CTRL>(a.s);
    const int bidx = __builtin_amdgcn_update_dpp(0, a.idx, CTRL, 0xF, 0xF, true);
    score_merge(a, bm, bs, bidx);
}
__device__ __forceinline__ void score_merge_xor(ScoreAcc &a, int o) {
    const float bm = __shfl_xor(a.m, o);
    const double bs = __shfl_xor(a.s, o);
    const int bidx = __shfl_xor(a.idx, o);
    score_merge(a, bm, bs, bidx);
}

struct ScoreRowsParams {
    const float *logits;   // [n][ld]
    long long ld;          // floats between rows
    int vocab;
    const int *targets;    // [n]: id whose log-probability is wanted, -1: none
    float *logprob;        // [n]
    float *lse;            // [n] or nullptr
    int *argmax;           // [n] or nullptr
};

constexpr int SCORE_THREADS = 1024;

// One workgroup per row, one pass: every entry is loaded once, 16 bytes per lane over the aligned body of the row, one
// entry per lane over the <= 3 entries in front of the first 16-byte boundary and the <= 3 behind the last.  A thread keeps
// (m, s) online -- a group of four entries raises m at most once, so it costs four exponentials and, while the maximum
// still moves, a fifth -- and the entry at the target index is handed over through LDS by the thread that loaded it.
// Merge order (fixed, so a replay is bitwise equal): lanes by the butterfly xor 1, 2, 4 (half mirror), 8 (row mirror) on DPP,
// then xor 16, 32; wavefronts 0 .. 15 in ascending order by thread 0 through LDS.
__global__ void __launch_bounds__(SCORE_THREADS) score_rows_kernel(ScoreRowsParams P) {
    __shared__ float w_m[SCORE_THREADS / 64];
    __shared__ double w_s[SCORE_THREADS / 64];
    __shared__ int w_idx[SCORE_THREADS / 64];
    __shared__ float s_xt;
    const int row = blockIdx.x, tid = threadIdx.x, V = P.vocab;
    const float *lg = P.logits + (long long)row * P.ld;
    const int t = P.targets[row];
    // entries in front of the first 16-byte boundary (the row base is 4-byte aligned), whole float4 groups, the rest
    const int head = min(V, (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(lg) >> 2) & 3u)) & 3u));
    const int n4 = (V - head) >> 2, tail0 = head + 4 * n4;
    ScoreAcc a{-INFINITY, 0.0, SCORE_NO_IDX};
    auto one = [&](int i) {
        const float v = lg[i];
        if (i == t) s_xt = v;
        if (v > a.m || (v == a.m && i < a.idx)) a.idx = i;
        if (v > a.m) { a.s = a.s * score_scale(a.m, v); a.m = v; }
        if (a.m != -INFINITY) a.s += score_scale(v, a.m);
    };
    if (tid < head) one(tid);
    if (tid < V - tail0) one(tail0 + tid);
    const float4 *body = reinterpret_cast<const float4 *>(lg + head);
    for (int g = tid; g < n4; g += SCORE_THREADS) {
        const float4 q = body[g];
        const int i = head + 4 * g;
        const float v[4] = {q.x, q.y, q.z, q.w};
        if ((unsigned)(t - i) < 4u) s_xt = v[t - i];
        float gm = a.m;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (v[j] > gm || (v[j] == gm && i + j < a.idx)) { gm = v[j]; a.idx = i + j; }
        if (gm > a.m) { a.s = a.s * score_scale(a.m, gm); a.m = gm; }
        if (a.m != -INFINITY) {
            const double md = (double)a.m;
            double e0 = exp_f64_chain((double)v[0] - md), e1 = exp_f64_chain((double)v[1] - md);
            double e2 = exp_f64_chain((double)v[2] - md), e3 = exp_f64_chain((double)v[3] - md);
            a.s += (e0 + e1) + (e2 + e3);
        }
    }
    score_merge_dpp<DPP_QUAD_XOR1>(a);
    score_merge_dpp<DPP_QUAD_XOR2>(a);
    score_merge_dpp<DPP_HALF_MIRROR>(a);
    score_merge_dpp<DPP_ROW_MIRROR>(a);
    score_merge_xor(a, 16);
    score_merge_xor(a, 32);
    if ((tid & 63) == 0) { w_m[tid >> 6] = a.m; w_s[tid >> 6] = a.s; w_idx[tid >> 6] = a.idx; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SCORE_THREADS / 64; w++) score_merge(a, w_m[w], w_s[w], w_idx[w]);
        const double lse = (double)a.m + log(a.s);      // (every entry -inf: -inf + log 0 = -inf)
        if (P.lse) P.lse[row] = (float)lse;
        if (P.argmax) P.argmax[row] = a.idx == SCORE_NO_IDX ? 0 : a.idx;
        P.logprob[row] = t >= 0 && t < V ? (float)((double)s_xt - lse) : 0.0f;
    }
}

inline hipError_t launch_score_rows(const ScoreRowsParams &P, int n, hipStream_t st) {
    hipLaunchKernelGGL(score_rows_kernel, dim3(n), dim3(SCORE_THREADS), 0, st, P);
    return hipGetLastError();
}

}  // namespace nl
