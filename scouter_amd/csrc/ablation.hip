// Ablation-CAM (Desai & Ramaswamy, WACV 2020): the gradient-free class activation map.  Every channel of the backbone's output is
// zeroed in turn, the ablated features go through the head alone, and a channel's weight is the relative drop of the class
// probability.  Two kernels, each with one fixed order per output element and no atomics, so two calls give the same bits.
//
// ablate_channels_kernel: feat NHWC [P][C] -> out [1 + n][P][C]; row 0 is feat, row 1 + j is feat with channel first + j set to 0.0f at
//   every position -- a select, every other value an exact copy.  A workgroup belongs to ONE row (blockIdx.x); it reads the
//   features (L2-resident after the first row) and writes its row once: the kernel is HBM stores.  C a multiple of 4 and 16-byte
//   aligned pointers: four channels of a position per thread, 16-byte loads and stores; anything else: one element per thread.
// ablation_contract_kernel: out[k][p] = sum_c w[k][c] feat[p][c], w[k][c] = (float)(deltas[k][c] / exp((double)clean[cols[k]])),
//   rounded from fp64 once.  One thread per position and per tile of AB_KT classes (blockIdx.y), AB_KT accumulators in registers
//   that start at 0 and take one fma per channel in ascending order (at_fma_tile), clamped at 0 at the end with `relu`.  The
//   weights of AB_NP channels at a time are staged in LDS, so C is unbounded.
#include "attr_common.h"

constexpr int AB_THREADS = 256;
constexpr int AB_KT = 16;                     // classes per thread (accumulators in registers)
constexpr int AB_NP = 32;                     // channels whose weights are staged in LDS at a time

static int ab_check_features(const char* what, long P, int C) {
    SC_REQUIRE(P > 0 && C > 0, "%s: bad arguments (P %ld positions, C %d channels: each must be at least 1)", what, P, C);
    SC_UNSUPPORTED(P * C < (1L << 31), "%s: features of %ld x %d elements are past the 32-bit offsets", what, P, C);
    return SC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(AB_THREADS) void ablate_channels_kernel(const float* __restrict__ feat, float* __restrict__ out,
                                                                     int first, int P, int C) {
    const int r = blockIdx.x, tid = threadIdx.x;
    const int gone = r > 0 ? first + r - 1 : -1;               // (row 0: the features themselves)
    float* __restrict__ o = out + (long)r * P * C;
    constexpr int V = VEC ? 4 : 1;
    const int cq = C / V;                                       // (VEC: C is a multiple of 4)
    const long items = (long)P * cq;
    for (long i = (long)blockIdx.y * AB_THREADS + tid; i < items; i += (long)gridDim.y * AB_THREADS) {
        const long e = i * V;                                   // (positions are whole groups of V: flat index = V i)
        const int c = (int)(i % cq) * V;
        float v[V];
        at_load<V>(feat + e, v);
#pragma unroll
        for (int k = 0; k < V; ++k) v[k] = c + k == gone ? 0.f : v[k];
        if constexpr (VEC) *(f32x4*)(o + e) = f32x4{v[0], v[1], v[2], v[3]};
        else o[e] = v[0];
    }
}

extern "C" int scouter_ablate_channels_f32(const float* feat, float* out, int first, int n, int P, int C, void* stream) {
    SC_REQUIRE(feat && out, "ablate_channels: null pointer (feat %p, out %p)", (const void*)feat, (void*)out);
    SC_REQUIRE((((uintptr_t)feat | (uintptr_t)out) & 3) == 0,
               "ablate_channels: misaligned pointer (feat and out must be 4-byte aligned)");
    SC_REQUIRE(n > 0, "ablate_channels: bad arguments (n %d must be at least 1)", n);
    if (int rc = ab_check_features("ablate_channels", P, C)) return rc;
    SC_REQUIRE(first >= 0 && (long)first + n <= C, "ablate_channels: channels [%d, %ld) lie outside [0, C = %d)", first,
               (long)first + n, C);
    hipStream_t st = (hipStream_t)stream;
    const AtPixelGrid px = at_pixel_grid(P, C, AB_THREADS, (uintptr_t)feat | (uintptr_t)out);
    const double elems = (1.0 + n) * P * C;
    ScProfScope prof("ablate_channels", st, elems, 4.0 * (elems + (double)P * C));
    const dim3 grid((unsigned)(1 + n), px.tiles);
    if (px.vec) hipLaunchKernelGGL(ablate_channels_kernel<true>, grid, dim3(AB_THREADS), 0, st, feat, out, first, P, C);
    else hipLaunchKernelGGL(ablate_channels_kernel<false>, grid, dim3(AB_THREADS), 0, st, feat, out, first, P, C);
    return sc_check_launch("ablate_channels");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(AB_THREADS) void ablation_contract_kernel(const double* __restrict__ deltas,
                                                                       const float* __restrict__ clean,
                                                                       const int* __restrict__ cols, const float* __restrict__ feat,
                                                                       float* __restrict__ out, int K, int n_classes, int P, int C,
                                                                       int relu) {
    __shared__ __attribute__((aligned(16))) float s_w[AB_NP][AB_KT];
    __shared__ double s_den[AB_KT];
    const int tid = threadIdx.x;
    const int k0 = blockIdx.y * AB_KT, kt = min(AB_KT, K - k0);
    if (tid < AB_KT) {                                          // (the caller refuses an index outside [0, n_classes))
        const int col = min(max(tid < kt ? cols[k0 + tid] : 0, 0), n_classes - 1);
        s_den[tid] = exp((double)clean[col]);
    }
    const int p = blockIdx.x * AB_THREADS + tid;
    const bool mine = p < P;
    const float* __restrict__ f = feat + (long)(mine ? p : 0) * C;
    float a[AB_KT];
#pragma unroll
    for (int k = 0; k < AB_KT; ++k) a[k] = 0.f;

    for (int c0 = 0; c0 < C; c0 += AB_NP) {
        const int np = min(AB_NP, C - c0);
        __syncthreads();                                        // (s_den is written; the previous piece is consumed)
        for (int i = tid; i < AB_NP * AB_KT; i += AB_THREADS) {
            const int k = i / AB_NP, j = i - k * AB_NP;         // (consecutive threads read consecutive channels of a class)
            s_w[j][k] = (k < kt && j < np) ? (float)(deltas[(long)(k0 + k) * C + c0 + j] / s_den[k]) : 0.f;
        }
        __syncthreads();
        if (mine)
            for (int j = 0; j < np; ++j) at_fma_tile<AB_KT>(s_w[j], f[c0 + j], a);
    }
    if (mine) {
        if (relu) {
#pragma unroll
            for (int k = 0; k < AB_KT; ++k) a[k] = fmaxf(a[k], 0.f);
        }
        at_store_acc<AB_KT>(out, P, p, k0, kt, a);
    }
}

extern "C" int scouter_ablation_contract_f32(const double* deltas, const float* clean, const int* cols, const float* feat, float* out,
                                             int K, int n_classes, int P, int C, int relu, void* stream) {
    SC_REQUIRE(deltas && clean && cols && feat && out,
               "ablation_contract: null pointer (deltas %p, clean %p, cols %p, feat %p, out %p)", (const void*)deltas,
               (const void*)clean, (const void*)cols, (const void*)feat, (void*)out);
    SC_REQUIRE((((uintptr_t)clean | (uintptr_t)cols | (uintptr_t)feat | (uintptr_t)out) & 3) == 0 && ((uintptr_t)deltas & 7) == 0,
               "ablation_contract: misaligned pointer (clean, cols, feat and out must be 4-byte aligned, deltas 8-byte)");
    SC_REQUIRE(K > 0 && n_classes > 0, "ablation_contract: bad arguments (K %d, n_classes %d: each must be at least 1)", K,
               n_classes);
    if (int rc = ab_check_features("ablation_contract", P, C)) return rc;
    const int ktiles = sc_cdiv(K, AB_KT);
    SC_UNSUPPORTED(ktiles <= 65535, "ablation_contract: K = %d classes (at most %d)", K, 65535 * AB_KT);
    SC_UNSUPPORTED((long)C * K < (1L << 31), "ablation_contract: weights of %d x %d elements are past the 32-bit offsets", K, C);
    hipStream_t st = (hipStream_t)stream;
    const double px = (double)P;
    ScProfScope prof("ablation_contract", st, 2.0 * C * px * ktiles * AB_KT, 4.0 * K * px + 8.0 * C * K + 4.0 * C * px);
    hipLaunchKernelGGL(ablation_contract_kernel, dim3((unsigned)sc_cdiv(P, AB_THREADS), (unsigned)ktiles), dim3(AB_THREADS), 0, st,
                       deltas, clean, cols, feat, out, K, n_classes, P, C, relu);
    return sc_check_launch("ablation_contract");
}
