// Training augmentation on the GPU (`--aug true`; the reference's tools/image_aug.py, an imgaug Sequential of Fliplr, Flipud,
// Affine and GaussianBlur in random order, applied per image on a CPU worker between Resize and ToTensor).  The definition --
// parameter ranges, the reduction of a drawn sequence to blur_first / warp / blur_last, the arithmetic of every stage and
// the departures from imgaug / OpenCV -- is the docstring of scouter_amd/dataset/augment.py; `augment_host` there is the
// yardstick.  Here: three byte-streaming kernels on planar bytes [B][C][S][S].  Which stage an image takes is decided IN
// the kernels from a per-image parameter table on the device (klen 0 = copy, identity flag = copy), so a batch is one
// launch per stage whatever was drawn, and the host never reads anything back.
//   aug_blur_kernel    one launch for both passes: a workgroup loads a 64 x 32 tile plus its halo of 4 (reflect-101)
//                      into LDS as bytes, writes the row pass into LDS as float and runs the column pass from LDS -- the
//                      unrounded intermediate never reaches HBM.  Lanes run along x in all three phases.
//   aug_warp_kernel    inverse-mapped bilinear sampling, zeros outside; the coordinates are computed once per pixel and
//                      used for every channel.
//   aug_finish_kernel  ToTensor + Normalize as the [C][256] table lookup (table in LDS), 4 bytes in, one float4 out.
#include "common.h"

#define AUG_TW 64
#define AUG_TH 32
#define AUG_HALO 4
#define AUG_MAX_KLEN (2 * AUG_HALO + 1)

__device__ __forceinline__ unsigned char aug_byte(float v) {
    v = rintf(v);                                             // half to even
    return (unsigned char)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));
}

// reflect-101 (index -i reads i, S-1+i reads S-1-i), then clamped: positions of a partial tile beyond the image's own
// halo are never used, they only have to stay inside the plane
__device__ __forceinline__ int aug_reflect(int g, int S) {
    if (g < 0) g = -g;
    if (g > S - 1) g = 2 * (S - 1) - g;
    return g < 0 ? 0 : (g > S - 1 ? S - 1 : g);
}

// grid (ceil(S / 64), ceil(S / 32), B * C)
__global__ __launch_bounds__(256) void aug_blur_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                       const int* __restrict__ klen_tab, int klen_stride,
                                                       const float* __restrict__ taps_tab, int taps_stride, int C, int S) {
    __shared__ unsigned char tile[AUG_TH + 2 * AUG_HALO][AUG_TW + 2 * AUG_HALO];
    __shared__ float rows[AUG_TH + 2 * AUG_HALO][AUG_TW];
    __shared__ float tp[AUG_MAX_KLEN];
    const int b = blockIdx.z / C;
    const int x0 = blockIdx.x * AUG_TW, y0 = blockIdx.y * AUG_TH;
    const long plane = (long)blockIdx.z * S * S;
    int klen = klen_tab[(long)b * klen_stride];               // the same for the whole workgroup
    klen = klen > AUG_MAX_KLEN ? AUG_MAX_KLEN : klen;
    if (klen <= 0) {                                          // this image does not blur at this stage: copy
        for (int it = threadIdx.x; it < AUG_TH * AUG_TW; it += 256) {
            const int y = y0 + it / AUG_TW, x = x0 + it % AUG_TW;
            if (y < S && x < S) dst[plane + (long)y * S + x] = src[plane + (long)y * S + x];
        }
        return;
    }
    const int r = klen >> 1;
    if (threadIdx.x < klen) tp[threadIdx.x] = taps_tab[(long)b * taps_stride + threadIdx.x];
    for (int it = threadIdx.x; it < (AUG_TH + 2 * AUG_HALO) * (AUG_TW + 2 * AUG_HALO); it += 256) {
        const int ly = it / (AUG_TW + 2 * AUG_HALO), lx = it % (AUG_TW + 2 * AUG_HALO);
        const int gy = aug_reflect(y0 + ly - AUG_HALO, S), gx = aug_reflect(x0 + lx - AUG_HALO, S);
        tile[ly][lx] = src[plane + (long)gy * S + gx];
    }
    __syncthreads();
    for (int it = threadIdx.x; it < (AUG_TH + 2 * AUG_HALO) * AUG_TW; it += 256) {      // row pass, halo rows included
        const int ly = it / AUG_TW, lx = it % AUG_TW;
        float acc = 0.f;
        for (int i = 0; i < klen; ++i) acc += tp[i] * (float)tile[ly][lx + AUG_HALO - r + i];
        rows[ly][lx] = acc;
    }
    __syncthreads();
    for (int it = threadIdx.x; it < AUG_TH * AUG_TW; it += 256) {                         // column pass
        const int ly = it / AUG_TW, lx = it % AUG_TW;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= S || x >= S) continue;
        float acc = 0.f;
        for (int i = 0; i < klen; ++i) acc += tp[i] * rows[ly + AUG_HALO - r + i][lx];
        dst[plane + (long)y * S + x] = aug_byte(acc);
    }
}

#pragma clang fp contract(off)
// source coordinate of output pixel (x, y): two rounded products, their rounded sum, the rounded sum with the constant --
// the steps the definition names, so that host and device agree on every bit of it
__device__ __forceinline__ float aug_coord(float a, float b, float c, float x, float y) {
    const float p = a * x, q = b * y;
    const float s = p + q;
    return s + c;
}
#pragma clang fp contract(fast)

__device__ __forceinline__ float aug_tap(const unsigned char* __restrict__ p, int y, int x, int S) {
    return ((unsigned)x < (unsigned)S && (unsigned)y < (unsigned)S) ? (float)p[(long)y * S + x] : 0.f;
}

// grid (ceil(S / 64), ceil(S / 4), B); block 64 x 4
__global__ __launch_bounds__(256) void aug_warp_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                       const float* __restrict__ minv_tab, int minv_stride,
                                                       const int* __restrict__ ident_tab, int ident_stride, int C, int S) {
    const int b = blockIdx.z;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= S || y >= S) return;
    const long image = (long)b * C * S * S, at = (long)y * S + x;
    if (ident_tab[(long)b * ident_stride]) {
        for (int c = 0; c < C; ++c) dst[image + (long)c * S * S + at] = src[image + (long)c * S * S + at];
        return;
    }
    const float* __restrict__ m = minv_tab + (long)b * minv_stride;
    const float u = aug_coord(m[0], m[1], m[2], (float)x, (float)y), v = aug_coord(m[3], m[4], m[5], (float)x, (float)y);
    const float fu = floorf(u), fv = floorf(v);
    const float ax = u - fu, ay = v - fv;
    // (a coordinate far outside -- or a NaN from a broken matrix -- must not wrap into the image when it becomes an int)
    const bool far = !(fu >= -2.f && fu <= (float)S && fv >= -2.f && fv <= (float)S);
    const int xs = far ? -2 : (int)fu, ys = far ? -2 : (int)fv;
    for (int c = 0; c < C; ++c) {
        const unsigned char* __restrict__ p = src + image + (long)c * S * S;
        const float top = aug_tap(p, ys, xs, S) * (1.f - ax) + aug_tap(p, ys, xs + 1, S) * ax;
        const float bottom = aug_tap(p, ys + 1, xs, S) * (1.f - ax) + aug_tap(p, ys + 1, xs + 1, S) * ax;
        dst[image + (long)c * S * S + at] = aug_byte(top * (1.f - ay) + bottom * ay);
    }
}

// out[b][c][y][x] = lut[c][src[b][c][y][x]];  `quads`: plane size is a multiple of 4, a thread converts 4 bytes at once
__global__ __launch_bounds__(256) void aug_finish_kernel(const unsigned char* __restrict__ src, const float* __restrict__ lut,
                                                         float* __restrict__ out, int C, long plane, long total, int quads) {
    __shared__ float tab[4 * 256];
    for (int i = threadIdx.x; i < C * 256; i += 256) tab[i] = lut[i];
    __syncthreads();
    const long step = (long)gridDim.x * 256;
    if (quads) {
        for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total / 4; q += step) {
            const float* __restrict__ t = tab + ((q * 4 / plane) % C) * 256;
            const unsigned w = *(const unsigned*)(src + q * 4);
            *(f32x4*)(out + q * 4) = f32x4{t[w & 255u], t[(w >> 8) & 255u], t[(w >> 16) & 255u], t[w >> 24]};
        }
    } else {
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += step)
            out[i] = tab[((i / plane) % C) * 256 + src[i]];
    }
}

static int aug_shape_ok(const char* what, int B, int C, int S) {
    if (B > 0 && (C == 1 || C == 3 || C == 4) && S >= 5 && S <= 32768 && (long)B * C <= 65535 && B <= 65535) return 1;
    sc_set_error("%s: bad shape B=%d C=%d S=%d (C in {1, 3, 4}, 5 <= S <= 32768, B * C <= 65535)", what, B, C, S);
    return 0;
}

extern "C" int scouter_aug_blur_u8(const unsigned char* src, unsigned char* dst, const int* klen, int klen_stride,
                                   const float* taps, int taps_stride, int B, int C, int S, void* stream) {
    SC_REQUIRE(src && dst && klen && taps, "aug_blur: null pointer");
    SC_REQUIRE(src != dst, "aug_blur: in-place blur is not possible (tiles read their neighbours' bytes)");
    if (!aug_shape_ok("aug_blur", B, C, S)) return SC_ERR_ARG;
    SC_REQUIRE(klen_stride >= 1 && taps_stride >= AUG_MAX_KLEN, "aug_blur: bad table strides %d, %d", klen_stride, taps_stride);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("aug_blur", st, 4.0 * AUG_MAX_KLEN * B * C * S * S, 2.0 * B * C * S * S);
    hipLaunchKernelGGL(aug_blur_kernel, dim3(sc_cdiv(S, AUG_TW), sc_cdiv(S, AUG_TH), B * C), dim3(256), 0, st, src, dst, klen,
                       klen_stride, taps, taps_stride, C, S);
    return sc_check_launch("aug_blur");
}

extern "C" int scouter_aug_warp_u8(const unsigned char* src, unsigned char* dst, const float* minv, int minv_stride,
                                   const int* identity, int identity_stride, int B, int C, int S, void* stream) {
    SC_REQUIRE(src && dst && minv && identity, "aug_warp: null pointer");
    SC_REQUIRE(src != dst, "aug_warp: in-place warp is not possible");
    if (!aug_shape_ok("aug_warp", B, C, S)) return SC_ERR_ARG;
    SC_REQUIRE(minv_stride >= 6 && identity_stride >= 1, "aug_warp: bad table strides %d, %d", minv_stride, identity_stride);
    hipStream_t st = (hipStream_t)stream;
    ScProfScope prof("aug_warp", st, 14.0 * B * C * S * S, 5.0 * B * C * S * S);
    hipLaunchKernelGGL(aug_warp_kernel, dim3(sc_cdiv(S, 64), sc_cdiv(S, 4), B), dim3(256), 0, st, src, dst, minv, minv_stride,
                       identity, identity_stride, C, S);
    return sc_check_launch("aug_warp");
}

extern "C" int scouter_aug_finish_u8_f32(const unsigned char* src, const float* lut, float* out, int B, int C, int S,
                                         void* stream) {
    SC_REQUIRE(src && lut && out, "aug_finish: null pointer");
    SC_REQUIRE(B > 0 && (C == 1 || C == 3 || C == 4) && S > 0, "aug_finish: bad shape B=%d C=%d S=%d", B, C, S);
    hipStream_t st = (hipStream_t)stream;
    const long plane = (long)S * S, total = plane * C * B;
    const int quads = plane % 4 == 0 && ((uintptr_t)src % 4 == 0) && ((uintptr_t)out % 16 == 0);
    ScProfScope prof("aug_finish", st, 0, 5.0 * total);
    const long work = quads ? total / 4 : total;
    const int blocks = (int)(work / 256 + 1 < 4096 ? work / 256 + 1 : 4096);
    hipLaunchKernelGGL(aug_finish_kernel, dim3(blocks), dim3(256), 0, st, src, lut, out, C, plane, total, quads);
    return sc_check_launch("aug_finish");
}
