// Input gradient of the stem convolution (Cin < 32): dx[B][Cin][H][W] (NCHW fp32, the image layout) from
// dy[B][Ho][Wo][Cout] (NHWC fp32) and w (HWIO) -- what attribution maps read (d output / d image; reference
// train.py --grad, captum_vis.py).  Gather form: every dx element is ONE fixed-order sum over its taps and over Cout, no
// atomics, so the result is bit-identical run to run.
//
// Why direct: with Cin <= 3 a GEMM + col2im route would write and re-read a [M][Kpad] patch-gradient matrix (560 MB at
// 70 x 224^2 for the 7x7 stem); this kernel reads dy once (plus its tile halo, from L2) and writes dx once.
//
// stem_dgrad_s2_kernel (stride 2; Cin 1 / 3; 7x7 pad 3 and 3x3 pad 1; Cout a multiple of 16): a workgroup owns a
// 16 x 32 tile of dx for all Cin channels and walks Cout in chunks of 16: the dy tile with its halo
// ((8 + halo) x (16 + halo) pixels x 16 channels, pixel stride padded to 20 floats so that the 16 lanes of a row read 16
// disjoint bank groups with one 16-byte read each) and the chunk's weights ([k][k][Cin][16]) are staged in LDS -- 26 KB
// for the 7x7 stem, six workgroups per CU.  Out-of-range dy pixels are staged as zeros, so the tap loops have no bounds
// tests.  A stride-2 transposed convolution uses, for an output row y, only the filter rows ky = (y + pad) mod 2 (mod 2):
// a wave owns rows of ONE parity (wave-uniform tap set, compile-time trip counts), a lane owns the pixel pair
// (x0, x0 + 1), x0 even -- the two column parities, whose taps read the same halo + 1 dy columns -- and stores it as one
// 8-byte word: a wave's store covers 128 consecutive bytes of each of its four rows.
// stem_dgrad_generic_kernel: every other supported shape (Cin < 32, stride 1 or 2, k <= 11, pad < k), one thread per dx
// element with the tap tests in the loop.
#include "common.h"

constexpr int SD_TH = 16, SD_TW = 32, SD_CO = 16, SD_COP = SD_CO + 4;
typedef float sd_f32x2 __attribute__((ext_vector_type(2)));

// Stride 2.  A coordinate v = 2 m + q (parity q) receives the filter taps k = r + 2 t, r = (q + PAD) mod 2, t = 0 .. n - 1,
// from the source coordinate m + e - t, e = (q + PAD - r) / 2.  [lo, hi]: the source offsets (relative to m) either parity reads.
template <int K, int PAD>
struct SdTaps {
    static constexpr int r(int q) { return (q + PAD) & 1; }
    static constexpr int n(int q) { return (K - r(q) + 1) / 2; }
    static constexpr int e(int q) { return (q + PAD - r(q)) / 2; }
    static constexpr int lo0 = e(0) - (n(0) - 1), lo1 = e(1) - (n(1) - 1);
    static constexpr int lo = lo0 < lo1 ? lo0 : lo1;
    static constexpr int hi = e(0) > e(1) ? e(0) : e(1);
    static constexpr int halo = hi - lo;
};

template <int CIN, int K, int PAD, int PY>
__device__ __forceinline__ void stem_dgrad_taps(const float* __restrict__ s_dy, const float* __restrict__ s_w, int yl, int lx,
                                                float (&acc)[2][CIN]) {
    using T = SdTaps<K, PAD>;
    constexpr int COLS = SD_TW / 2 + T::halo;
    constexpr int NY = T::n(PY), RY = T::r(PY), EY = T::e(PY);
    const int rbase = (yl >> 1) + EY - T::lo;
#pragma unroll
    for (int t = 0; t < NY; ++t) {
        const int ky = RY + 2 * t;
        const float* row = s_dy + ((rbase - t) * COLS + lx) * SD_COP;
#pragma unroll
        for (int cq = 0; cq < SD_CO / 4; ++cq) {
            f32x4 d[T::halo + 1];
#pragma unroll
            for (int j = 0; j <= T::halo; ++j) d[j] = *(const f32x4*)(row + j * SD_COP + 4 * cq);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
#pragma unroll
                for (int tt = 0; tt < T::n(q); ++tt) {
                    const int kx = T::r(q) + 2 * tt, j = T::e(q) - tt - T::lo;
#pragma unroll
                    for (int c = 0; c < CIN; ++c) {
                        const f32x4 wv = *(const f32x4*)(s_w + ((ky * K + kx) * CIN + c) * SD_CO + 4 * cq);
                        float a = acc[q][c];
#pragma unroll
                        for (int i = 0; i < 4; ++i) a = fmaf(d[j][i], wv[i], a);
                        acc[q][c] = a;
                    }
                }
            }
        }
    }
}

template <int CIN, int K, int PAD>
__global__ __launch_bounds__(256) void stem_dgrad_s2_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                            float* __restrict__ dx, int H, int W, int Ho, int Wo, int Cout,
                                                            int tiles_x, int tiles_y) {
    using T = SdTaps<K, PAD>;
    constexpr int ROWS = SD_TH / 2 + T::halo, COLS = SD_TW / 2 + T::halo;
    __shared__ __attribute__((aligned(16))) float s_dy[ROWS * COLS * SD_COP];
    __shared__ __attribute__((aligned(16))) float s_w[K * K * CIN * SD_CO];
    const int bid = blockIdx.x;
    const int tx = bid % tiles_x, ty = (bid / tiles_x) % tiles_y, b = bid / (tiles_x * tiles_y);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int py = wv & 1, lx = lane & 15;
    const int yl = 2 * ((wv >> 1) * 4 + (lane >> 4)) + py;                       // row of the tile, parity py
    const int my0 = ty * (SD_TH / 2) + T::lo, mx0 = tx * (SD_TW / 2) + T::lo;    // dy coordinates of the staged tile's corner
    const float* dyb = dy + (long)b * Ho * Wo * Cout;
    float acc[2][CIN];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int c = 0; c < CIN; ++c) acc[q][c] = 0.f;
    for (int c0 = 0; c0 < Cout; c0 += SD_CO) {
        __syncthreads();                                                         // (the previous chunk has been consumed)
        for (int i = tid; i < ROWS * COLS * (SD_CO / 4); i += 256) {
            const int q = i & 3, p = i >> 2, r = p / COLS, c = p - r * COLS;
            const int oy = my0 + r, ox = mx0 + c;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) v = *(const f32x4*)(dyb + ((long)oy * Wo + ox) * Cout + c0 + 4 * q);
            *(f32x4*)(s_dy + p * SD_COP + 4 * q) = v;
        }
        for (int i = tid; i < K * K * CIN * (SD_CO / 4); i += 256) {
            const int q = i & 3, t = i >> 2;
            *(f32x4*)(s_w + t * SD_CO + 4 * q) = *(const f32x4*)(w + (long)t * Cout + c0 + 4 * q);
        }
        __syncthreads();
        if (py) stem_dgrad_taps<CIN, K, PAD, 1>(s_dy, s_w, yl, lx, acc);
        else stem_dgrad_taps<CIN, K, PAD, 0>(s_dy, s_w, yl, lx, acc);
    }
    const int y = ty * SD_TH + yl, x0 = tx * SD_TW + 2 * lx;
    if (y >= H || x0 >= W) return;
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
        float* p = dx + (((long)b * CIN + c) * H + y) * W + x0;
        if (x0 + 1 < W && (W & 1) == 0) {
            *(sd_f32x2*)p = sd_f32x2{acc[0][c], acc[1][c]};
        } else {
            p[0] = acc[0][c];
            if (x0 + 1 < W) p[1] = acc[1][c];
        }
    }
}

__global__ __launch_bounds__(256) void stem_dgrad_generic_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                 float* __restrict__ dx, long n, int Cin, int H, int W, int Ho,
                                                                 int Wo, int Cout, int k, int stride, int pad) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), c = (int)((i / ((long)W * H)) % Cin);
    const long b = i / ((long)W * H * Cin);
    float a = 0.f;
    for (int ky = 0; ky < k; ++ky) {
        const int sy = y + pad - ky;
        if (sy < 0 || sy % stride != 0 || sy / stride >= Ho) continue;
        for (int kx = 0; kx < k; ++kx) {
            const int sx = x + pad - kx;
            if (sx < 0 || sx % stride != 0 || sx / stride >= Wo) continue;
            const float* d = dy + ((b * Ho + sy / stride) * Wo + sx / stride) * Cout;
            const float* wp = w + ((long)(ky * k + kx) * Cin + c) * Cout;
            for (int co = 0; co < Cout; ++co) a = fmaf(d[co], wp[co], a);
        }
    }
    dx[i] = a;
}

template <int CIN, int K, int PAD>
static void stem_dgrad_s2_launch(const float* dy, const float* w, float* dx, int B, int H, int W, int Ho, int Wo, int Cout,
                          hipStream_t st) {
    const int tiles_x = sc_cdiv(W, SD_TW), tiles_y = sc_cdiv(H, SD_TH);
    hipLaunchKernelGGL((stem_dgrad_s2_kernel<CIN, K, PAD>), dim3((unsigned)((long)B * tiles_x * tiles_y)), dim3(256), 0, st, dy,
                       w, dx, H, W, Ho, Wo, Cout, tiles_x, tiles_y);
}

extern "C" int scouter_stem_dgrad_f32(const float* dy, const float* w, float* dx, int B, int Cin, int H, int W, int Cout, int k,
                                      int stride, int pad, void* stream) {
    SC_REQUIRE(dy && w && dx && B > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0, "stem_dgrad: bad arguments");
    SC_UNSUPPORTED(Cin < 32, "stem_dgrad: built for the stem (Cin < 32, got %d); the other layers have scouter_conv2d_dgrad_f32", Cin);
    SC_UNSUPPORTED(stride == 1 || stride == 2, "stem_dgrad: stride %d (1 or 2)", stride);
    SC_UNSUPPORTED(k >= 1 && k <= 11 && pad >= 0 && pad < k, "stem_dgrad: kernel %d / pad %d (k <= 11, pad < k)", k, pad);
    SC_UNSUPPORTED(H + 2 * pad >= k && W + 2 * pad >= k, "stem_dgrad: image %d x %d smaller than the kernel", H, W);
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    const long n = (long)B * Cin * H * W;
    const long tiles = (long)B * sc_cdiv(W, SD_TW) * sc_cdiv(H, SD_TH);
    // (image bases are 64-bit; offsets inside one image, the tile count and the generic kernel's grid are 32-bit)
    SC_UNSUPPORTED((long)Ho * Wo * Cout < (1L << 31) && (long)Cin * H * W < (1L << 31) && tiles < (1L << 31) &&
                       (n + 255) / 256 < (1L << 31),
                   "stem_dgrad: tensor too large for 32-bit offsets (B %d, %d x %d, Cout %d)", B, H, W, Cout);
    hipStream_t st = (hipStream_t)stream;
    const bool tiled = stride == 2 && Cout % SD_CO == 0 && (Cin == 1 || Cin == 3) && ((k == 7 && pad == 3) || (k == 3 && pad == 1));
    const double taps = (double)k * k / (stride * stride);
    const double flops = 2.0 * (double)n * taps * Cout, bytes = 4.0 * ((double)B * Ho * Wo * Cout + (double)n);
    if (tiled) {
        ScProfScope prof(k == 7 ? "stem_dgrad<7x7/2>" : "stem_dgrad<3x3/2>", st, flops, bytes);
        if (k == 7 && Cin == 3) stem_dgrad_s2_launch<3, 7, 3>(dy, w, dx, B, H, W, Ho, Wo, Cout, st);
        else if (k == 7) stem_dgrad_s2_launch<1, 7, 3>(dy, w, dx, B, H, W, Ho, Wo, Cout, st);
        else if (Cin == 3) stem_dgrad_s2_launch<3, 3, 1>(dy, w, dx, B, H, W, Ho, Wo, Cout, st);
        else stem_dgrad_s2_launch<1, 3, 1>(dy, w, dx, B, H, W, Ho, Wo, Cout, st);
        return sc_check_launch("stem_dgrad");
    }
    ScProfScope prof("stem_dgrad<generic>", st, flops, bytes);
    hipLaunchKernelGGL(stem_dgrad_generic_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dy, w, dx, n, Cin, H, W, Ho,
                       Wo, Cout, k, stride, pad);
    return sc_check_launch("stem_dgrad");
}
