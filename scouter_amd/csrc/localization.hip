// Localisation scores of uint8 explanation maps and the joint byte scaling of a group of maps (tools/attribution.py localization,
// slot_maps; tools/explanation_table.py): two kernels, integer or single-rounding arithmetic per element and no atomics.
//
// map_localization_kernel: ONE workgroup of 1024 threads per map [H][W] of bytes.  A thread walks the map four pixels at a time
//   (one 4-byte load where the map starts on a 4-byte boundary and H W is a multiple of 4) and keeps three 64-bit integers:
//   the sum of its bytes, the sum of those inside the union of the image's boxes (clipped to the map and held in LDS, at most
//   32; a pixel under two boxes is tested until the first one that holds it, so it counts once), and the key
//   (byte << 32) | ~index, whose maximum is the largest byte at the smallest flat index.  The three meet in a butterfly and then
//   wave by wave through LDS.  Integers only: every value is exact whatever the order.
//
// group_maps_kernel: ONE workgroup of 256 threads per group of G maps [N]: the extrema of the G N values (at_block_minmax), then
//   out = (unsigned char)((v - lo) / span * 255.f) -- three correctly rounded fp32 operations in this order (nothing here can be
//   contracted into an fma), truncating -- what SlotAttention.vis_maps does on the host for one image.  span == 0: zeros.
#include "attr_common.h"

constexpr int LC_THREADS = 1024, LC_WAVES = LC_THREADS / 64, LC_MAX_BOXES = 32;
constexpr int GM_THREADS = 256, GM_WAVES = GM_THREADS / 64;

typedef unsigned long long lc_u64;

__device__ __forceinline__ bool lc_inside(const int* __restrict__ s_box, int nb, int y, int x) {
    for (int j = 0; j < nb; ++j)
        if (x >= s_box[4 * j] && x < s_box[4 * j + 2] && y >= s_box[4 * j + 1] && y < s_box[4 * j + 3]) return true;
    return false;
}

template <bool VEC>
__global__ __launch_bounds__(LC_THREADS) void map_localization_kernel(const unsigned char* __restrict__ maps,
                                                                      const int* __restrict__ boxes, const int* __restrict__ n_boxes,
                                                                      long* __restrict__ sums, int K, int H, int W, int max_boxes) {
    __shared__ int s_box[4 * LC_MAX_BOXES];
    __shared__ lc_u64 s_sum[LC_WAVES], s_in[LC_WAVES], s_key[LC_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.x / K, HW = H * W;
    const int nb = boxes && n_boxes ? min(max(n_boxes[b], 0), max_boxes) : 0;
    if (tid < nb) {                                                     // clipped to the map; an inverted box holds nothing
        const int* __restrict__ bx = boxes + ((long)b * max_boxes + tid) * 4;
        s_box[4 * tid] = max(bx[0], 0);
        s_box[4 * tid + 1] = max(bx[1], 0);
        s_box[4 * tid + 2] = min(bx[2], W);
        s_box[4 * tid + 3] = min(bx[3], H);
    }
    __syncthreads();
    const unsigned char* __restrict__ m = maps + (long)blockIdx.x * HW;
    constexpr int V = VEC ? 4 : 1;
    lc_u64 sum = 0, in = 0, key = 0;                                    // (key 0: below the key of every pixel, ~index >= 1)
    for (long i = V * tid; i < HW; i += V * LC_THREADS) {              // (long: the last stride steps past 2^31 at the largest map)
        unsigned word = VEC ? *(const unsigned*)(m + i) : (unsigned)m[i];
        int y = (int)(i / W), x = (int)(i - (long)y * W);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const unsigned v = word & 255u;
            word >>= 8;
            sum += v;
            if (nb && lc_inside(s_box, nb, y, x)) in += v;
            const lc_u64 cand = ((lc_u64)v << 32) | (lc_u64)(~(unsigned)(i + j));
            key = cand > key ? cand : key;
            if (++x == W) { x = 0; ++y; }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        in += __shfl_xor(in, o, 64);
        const lc_u64 other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
    }
    if (lane == 0) { s_sum[wv] = sum; s_in[wv] = in; s_key[wv] = key; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < LC_WAVES; ++k) {
            sum += s_sum[k];
            in += s_in[k];
            key = s_key[k] > key ? s_key[k] : key;
        }
        const int arg = (int)(~(unsigned)(key & 0xffffffffu));
        const int y = arg / W;
        long* __restrict__ o = sums + (long)blockIdx.x * 4;
        o[0] = (long)sum;
        o[1] = (long)in;
        o[2] = arg;
        o[3] = nb && lc_inside(s_box, nb, y, arg - y * W) ? 1 : 0;
    }
}

extern "C" int scouter_map_localization_u8(const unsigned char* maps, const int* boxes, const int* n_boxes, long* sums, int B,
                                           int K, int H, int W, int max_boxes, void* stream) {
    SC_REQUIRE(maps && sums, "map_localization: null pointer (maps %p, sums %p)", (const void*)maps, (void*)sums);
    SC_REQUIRE((boxes == nullptr) == (n_boxes == nullptr), "map_localization: boxes %p and n_boxes %p must both be given or both be null",
               (const void*)boxes, (const void*)n_boxes);
    SC_REQUIRE(B > 0 && K > 0 && H > 0 && W > 0 && max_boxes > 0,
               "map_localization: bad arguments (B %d, K %d, %d x %d, max_boxes %d: each must be at least 1)", B, K, H, W, max_boxes);
    SC_REQUIRE(((uintptr_t)boxes & 3) == 0 && ((uintptr_t)n_boxes & 3) == 0 && ((uintptr_t)sums & 7) == 0,
               "map_localization: misaligned pointer (boxes and n_boxes 4-byte, sums 8-byte aligned)");
    SC_UNSUPPORTED(max_boxes <= LC_MAX_BOXES, "map_localization: %d boxes an image (they live in LDS: at most %d)", max_boxes,
                   LC_MAX_BOXES);
    SC_UNSUPPORTED((long)H * W < (1L << 31) && (long)B * K < (1L << 31),
                   "map_localization: a map of %d x %d pixels or %d x %d maps are past the 32-bit offsets", H, W, B, K);
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)H * W;
    ScProfScope prof("map_localization", st, 4.0 * B * K * (double)HW, (double)B * K * ((double)HW + 32.0));
    const dim3 grid((unsigned)(B * K));
    if (((uintptr_t)maps & 3) == 0 && HW % 4 == 0)
        hipLaunchKernelGGL(map_localization_kernel<true>, grid, dim3(LC_THREADS), 0, st, maps, boxes, n_boxes, sums, K, H, W,
                           max_boxes);
    else
        hipLaunchKernelGGL(map_localization_kernel<false>, grid, dim3(LC_THREADS), 0, st, maps, boxes, n_boxes, sums, K, H, W,
                           max_boxes);
    return sc_check_launch("map_localization");
}

// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GM_THREADS) void group_maps_kernel(const float* __restrict__ maps, unsigned char* __restrict__ out,
                                                                long E) {
    __shared__ float s_lo[GM_WAVES], s_hi[GM_WAVES];
    const float* __restrict__ src = maps + (long)blockIdx.x * E;
    unsigned char* __restrict__ dst = out + (long)blockIdx.x * E;
    float lo = INFINITY, hi = -INFINITY;
    for (long i = threadIdx.x; i < E; i += GM_THREADS) {
        const float v = src[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    at_block_minmax<GM_WAVES>(lo, hi, s_lo, s_hi);
    const float span = hi - lo;
    const bool flat = !(span > 0.f);
    for (long i = threadIdx.x; i < E; i += GM_THREADS) {
        dst[i] = flat ? (unsigned char)0 : (unsigned char)(int)((src[i] - lo) / span * 255.f);
    }
}

extern "C" int scouter_group_maps_u8(const float* maps, unsigned char* out, int M, int G, long N, void* stream) {
    SC_REQUIRE(maps && out, "group_maps: null pointer (maps %p, out %p)", (const void*)maps, (void*)out);
    SC_REQUIRE(((uintptr_t)maps & 3) == 0, "group_maps: misaligned pointer (maps must be 4-byte aligned)");
    SC_REQUIRE(M > 0 && G > 0 && N > 0, "group_maps: bad arguments (M %d, G %d, N %ld: each must be at least 1)", M, G, N);
    SC_UNSUPPORTED(N < (1L << 31) && (long)G * N < (1L << 31), "group_maps: a group of %d x %ld values is past the 32-bit offsets", G, N);
    hipStream_t st = (hipStream_t)stream;
    const long E = (long)G * N;
    ScProfScope prof("group_maps", st, 3.0 * M * (double)E, 9.0 * M * (double)E);
    hipLaunchKernelGGL(group_maps_kernel, dim3((unsigned)M), dim3(GM_THREADS), 0, st, maps, out, E);
    return sc_check_launch("group_maps");
}
