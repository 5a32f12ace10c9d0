// nl_fork.h -- nl_kv_fork: the K / V rows [0, n_pos) of one stream copied into several others in ONE launch
// (KVCache.prefill, nanollama/engine.py:139-153: a batch-1 prefill's cache becomes every row of an N-row cache).
//
// The caches are [stream][layer][kv head][pos][head_dim] float32, so per (cache, layer, kv head) the rows [0, n_pos) are one
// contiguous run of n_pos * head_dim floats at the same offset inside every stream: a multiple of 128 bytes (head_dim is 32 or
// 64), 16-byte aligned everywhere.  A workgroup takes pieces of one run: every lane loads 16 bytes (a wavefront: 1 KiB
// contiguous), FORK_UNROLL loads in flight per lane, and stores each of them n_dst times -- the source is read once however
// many destinations there are.  The destination list travels in the argument block: no upload, nothing to wait for.
#pragma once
#include <hip/hip_runtime.h>

namespace nl {

constexpr int FORK_MAX_DST = 63;      // max_streams <= 64, one of them is the source
constexpr int FORK_THREADS = 256;
constexpr int FORK_UNROLL = 4;        // 16-byte loads in flight per lane: a piece is 256 * 4 * 16 B = 16 KiB
constexpr int FORK_MAX_GRID = 2048;   // workgroups of one launch (256 CUs x 8); the pieces beyond are strided over

struct KvForkParams {
    float *kcache, *vcache;           // [stream][layer][kv head][seq][hd]
    long long kv_stream_stride;       // floats per stream
    int run16;                        // 16-byte units of one run: n_pos * hd / 4
    int pitch16;                      // 16-byte units between the runs of one stream: seq_len * hd / 4
    int src, n_dst;
    int dst[FORK_MAX_DST];
};

// POLICY: 0 = plain loads and stores; 1 = non-temporal stores (the default: the copies are not read again before other
// traffic has passed through the caches; measured); 2 = non-temporal loads and stores (NL_FORK_POLICY)
template <int POLICY>
__device__ __forceinline__ uint4 fork_load(const uint4 *p) {
    if constexpr (POLICY >= 2) {
        typedef unsigned v4u __attribute__((ext_vector_type(4)));
        const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(p));
        return make_uint4(v.x, v.y, v.z, v.w);
    } else {
        return *p;
    }
}
template <int POLICY>
__device__ __forceinline__ void fork_store(uint4 *p, uint4 v) {
    if constexpr (POLICY >= 1) {
        typedef unsigned v4u __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(v4u{v.x, v.y, v.z, v.w}, reinterpret_cast<v4u *>(p));
    } else {
        *p = v;
    }
}

// grid (pieces, layers * kv heads, 2): blockIdx.z picks the cache, blockIdx.y the run, blockIdx.x strides over its pieces
template <int POLICY>
__global__ void __launch_bounds__(FORK_THREADS) kv_fork_kernel(KvForkParams P) {
    constexpr int PIECE = FORK_THREADS * FORK_UNROLL;
    float *cache = blockIdx.z ? P.vcache : P.kcache;
    uint4 *run = reinterpret_cast<uint4 *>(cache) + (long long)blockIdx.y * P.pitch16;     // stream 0's copy of this run
    const long long stride16 = P.kv_stream_stride / 4;
    const uint4 *src = run + P.src * stride16;
    for (int base = blockIdx.x * PIECE; base < P.run16; base += gridDim.x * PIECE) {
        uint4 v[FORK_UNROLL];
#pragma unroll
        for (int u = 0; u < FORK_UNROLL; u++) {
            const int i = base + u * FORK_THREADS + threadIdx.x;
            if (i < P.run16) v[u] = fork_load<POLICY>(src + i);
        }
        for (int d = 0; d < P.n_dst; d++) {
            uint4 *dst = run + P.dst[d] * stride16;
#pragma unroll
            for (int u = 0; u < FORK_UNROLL; u++) {
                const int i = base + u * FORK_THREADS + threadIdx.x;
                if (i < P.run16) fork_store<POLICY>(dst + i, v[u]);
            }
        }
    }
}

inline hipError_t launch_kv_fork(const KvForkParams &P, int n_runs, int policy, hipStream_t st) {
    constexpr int PIECE = FORK_THREADS * FORK_UNROLL;
    const int pieces = (P.run16 + PIECE - 1) / PIECE;
    const dim3 grid(std::max(1, std::min(pieces, FORK_MAX_GRID / (2 * n_runs))), n_runs, 2);
    if (policy >= 2) hipLaunchKernelGGL(kv_fork_kernel<2>, grid, dim3(FORK_THREADS), 0, st, P);
    else if (policy == 1) hipLaunchKernelGGL(kv_fork_kernel<1>, grid, dim3(FORK_THREADS), 0, st, P);
    else hipLaunchKernelGGL(kv_fork_kernel<0>, grid, dim3(FORK_THREADS), 0, st, P);
    return hipGetLastError();
}

}  // namespace nl
