// CAM of the FC baseline (Zhou et al., CVPR 2016; torchcam's CAM(model, 'layer4', 'fc') of the reference's torchcam_vis.py:
// CAM._get_weights followed by compute_cams): out[b][k][p] = sum_c w[col][c] feat[b][p][c], the fc weights of a class contracted
// with the last stage's features.  No bias, no 1 / N, no backward.
//
// cam_fc_kernel: ONE workgroup of 512 threads per image and tile of FC_PT = 8 positions.  The tile's features are staged in LDS
//   a piece of FC_CC = 2048 channels at a time ([8][2048] fp32 = 64 KiB: two workgroups a CU) and the K classes walk over the
//   piece, a wave per class: a lane reads its 16 bytes (VEC; 4 bytes otherwise) of the class's weight row once and multiplies
//   them onto the 8 positions in LDS, so the features of a launch cross HBM once and the weights come from L2 once per
//   workgroup.  At batch 70, 7 x 7 x 2048 and ten classes: 490 workgroups, 28 MB of features, 80 KB of weights.
//   Every class re-reads the piece from LDS, so for large K (200: 25 passes a wave) the LDS traffic sets the time, not HBM; with
//   K < 8 -- per_image has K = 1 -- all eight waves stage the piece and K of them contract it, the others wait at the barrier.
//   The order of one output element: a lane adds its channels of a piece in ascending order, one fma each, from 0 (VEC: the
//   four channels 4 q .. 4 q + 3 of the column groups q = lane, lane + 64, ...; otherwise the channels lane, lane + 64, ...);
//   the 64 partial sums meet in a butterfly; the pieces are added in ascending order onto the value the same lane left in `out`
//   after the piece before.  It depends on C alone -- not on B, K, per_image, or where the element sits in the batch, the tile
//   or the column list -- so two calls, a per-image call and the matching columns of an all-classes call give the same bits,
//   with no atomics.  At most C / 64 + 6 + C / 2048 roundings a term: below the worst case (C + 8) 2^-24 sum_c |w_c| |feat_c|.
#include "attr_common.h"

constexpr int FC_THREADS = 512, FC_WAVES = FC_THREADS / 64, FC_PT = 8, FC_CC = 2048;

template <bool VEC>
__global__ __launch_bounds__(FC_THREADS) void cam_fc_kernel(const float* __restrict__ feat, const float* __restrict__ w,
                                                            const int* __restrict__ cols, float* __restrict__ out, int N, int C,
                                                            int n_classes, int K, int ptiles, int per_image, int relu) {
    __shared__ __attribute__((aligned(16))) float s_feat[FC_PT * FC_CC];
    constexpr int V = VEC ? 4 : 1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x / ptiles, p0 = (blockIdx.x - b * ptiles) * FC_PT;
    const int pt = min(FC_PT, N - p0);
    const float* __restrict__ ft = feat + ((long)b * N + p0) * C;

    for (int c0 = 0; c0 < C; c0 += FC_CC) {
        const int cc = min(FC_CC, C - c0), groups = cc / V;             // (VEC: C and FC_CC are multiples of 4)
        if (c0) __syncthreads();                                        // the piece before has been read by every wave
        // ---- the piece [pt][cc] into LDS, rows pt .. FC_PT - 1 zero: every wave then runs the same FC_PT chains
        for (int i = tid; i < FC_PT * groups; i += FC_THREADS) {
            const int p = i / groups, q = i - p * groups;
            float v[V];
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = 0.f;
            if (p < pt) at_load<V, true>(ft + (long)p * C + c0 + V * q, v);
#pragma unroll
            for (int k = 0; k < V; ++k) s_feat[p * FC_CC + V * q + k] = v[k];
        }
        __syncthreads();

        // ---- a wave per class over the piece
        for (int k = wv; k < K; k += FC_WAVES) {
            const int col = min(max(cols[per_image ? b : k], 0), n_classes - 1);
            const float* __restrict__ wrow = w + (long)col * C + c0;
            float a[FC_PT];
#pragma unroll
            for (int p = 0; p < FC_PT; ++p) a[p] = 0.f;
            for (int q = lane; q < groups; q += 64) {
                float wq[V];
                at_load<V>(wrow + V * q, wq);
#pragma unroll
                for (int p = 0; p < FC_PT; ++p) {
                    float f[V];
                    at_load<V>(s_feat + p * FC_CC + V * q, f);
#pragma unroll
                    for (int j = 0; j < V; ++j) a[p] = fmaf(wq[j], f[j], a[p]);
                }
            }
            float mine = 0.f;                                           // lane p keeps position p0 + p
#pragma unroll
            for (int p = 0; p < FC_PT; ++p) {
                const float s = wave_sum(a[p]);
                if (lane == p) mine = s;
            }
            if (lane < pt) {
                float* __restrict__ o = out + ((long)b * K + k) * N + p0 + lane;
                if (c0) mine = *o + mine;
                if (relu && c0 + FC_CC >= C) mine = fmaxf(mine, 0.f);
                *o = mine;
            }
        }
    }
}

extern "C" int scouter_cam_fc_f32(const float* feat, const float* w, const int* cols, float* out, int B, int N, int C,
                                  int n_classes, int K, int per_image, int relu, void* stream) {
    SC_REQUIRE(feat && w && cols && out, "cam_fc: null pointer (feat %p, w %p, cols %p, out %p)", (const void*)feat,
               (const void*)w, (const void*)cols, (void*)out);
    SC_REQUIRE(B > 0 && N > 0 && C > 0 && n_classes > 0 && K > 0,
               "cam_fc: bad arguments (B %d, N %d, C %d, n_classes %d, K %d: each must be at least 1)", B, N, C, n_classes, K);
    SC_REQUIRE(!per_image || K == 1, "cam_fc: per-image columns give one map an image (K %d must be 1)", K);
    SC_REQUIRE(((uintptr_t)feat & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)cols & 3) == 0 && ((uintptr_t)out & 3) == 0,
               "cam_fc: misaligned pointer (feat and w 16-byte, cols and out 4-byte aligned)");
    const long ptiles = sc_cdiv(N, FC_PT);
    SC_UNSUPPORTED((long)B * N * C < (1L << 31) && (long)n_classes * C < (1L << 31) && (long)B * K * N < (1L << 31) &&
                       (long)B * ptiles < (1L << 31),
                   "cam_fc: features %d x %d x %d, weights %d x %d or maps %d x %d x %d are past the 32-bit offsets", B, N, C,
                   n_classes, C, B, K, N);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("cam_fc", st, 2.0 * B * (double)K * N * C, 4.0 * ((double)B * N * C + (double)B * ptiles * K * C + (double)B * K * N));
    const dim3 grid((unsigned)(B * ptiles));
    if (C % 4 == 0)
        hipLaunchKernelGGL(cam_fc_kernel<true>, grid, dim3(FC_THREADS), 0, st, feat, w, cols, out, N, C, n_classes, K, (int)ptiles,
                           per_image, relu);
    else
        hipLaunchKernelGGL(cam_fc_kernel<false>, grid, dim3(FC_THREADS), 0, st, feat, w, cols, out, N, C, n_classes, K, (int)ptiles,
                           per_image, relu);
    return sc_check_launch("cam_fc");
}
