// Calls every route query of include/scouter_hip.h over the threshold grid -- the shapes at which their 31 / 32-bit guards flip,
// where a product formed in int would overflow -- for a run under the undefined-behaviour sanitizer.  No device is needed: the
// queries are pure integer functions.  (Up to INT_MAX images, maps and channels: the queries answer 0 to sizes no tensor has before any product can overflow.)
// Host side of the library and this file with the sanitizer, from the repository root:
//   for f in scouter_amd/csrc/*.hip; do hipcc --offload-arch=gfx950 -O1 -std=c++17 -fPIC -Xarch_host -fsanitize=undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -c $f -o build_dev/ubsan/$(basename $f .hip).o; done
//   hipcc -std=c++17 -fsanitize=undefined -fno-sanitize-recover=undefined -Iinclude -x c++ -c tools_dev/route_queries_ubsan.cpp \
//       -o build_dev/ubsan/route_queries_main.o        (on its own: next to a .cpp, hipcc reads the object files as HIP source)
//   hipcc --offload-arch=gfx950 -fsanitize=undefined build_dev/ubsan/*.o -o build_dev/ubsan/route_queries_ubsan && \
//       build_dev/ubsan/route_queries_ubsan
#include <initializer_list>
#include <stdio.h>

extern "C" {
#include "scouter_hip.h"
}

int main() {
    static const int batches[] = {1, 2, 70, 668, 669, 1337, 1338, 2047, 2048, 4093, 4094, 4095, 4096, 16384, 16385, 65536, 1 << 20,
                                  1 << 24, 0x7fffffff};
    static const int maps[][2] = {{1, 1}, {2, 64}, {8, 8}, {32, 32}, {56, 56}, {64, 64}, {112, 112}, {16, 126}, {16, 127}, {2048, 2048}, {1 << 24, 1 << 24},
                                  {0x7fffffff, 0x7fffffff}};
    static const int chans[][3] = {{32, 32, 1}, {32, 64, 1}, {64, 256, 1}, {256, 64, 1}, {96, 128, 1}, {128, 256, 2}, {64, 64, 1},
                                   {1024, 512, 1}, {2048, 2048, 1}, {32768, 32768, 1},
                                   {1 << 20, 1 << 20, 1}, {0x7fffffe0, 0x7fffffe0, 1}};
    static const int filt[][4] = {{1, 1, 1, 0}, {3, 3, 1, 1}, {3, 3, 2, 1}, {5, 5, 1, 2}, {7, 7, 2, 3}, {3, 3, 1, 0x3fffffff}, {65535, 65535, 1, 65535}};
    long calls = 0, yes = 0;
    for (int B : batches)
        for (auto& m : maps)
            for (auto& c : chans)
                for (auto& f : filt) {
                    const int H = m[0], W = m[1], Ci = c[0], Co = c[1], g = c[2], kh = f[0], kw = f[1], s = f[2], p = f[3];
                    for (int tile = -1; tile <= 7; ++tile)
                        for (int epi = 0; epi < 64; epi += 7) {
                            yes += scouter_conv2d_fwd_tile_ok(B, H, W, Ci, Co, kh, kw, s, p, g, tile, epi);
                            yes += scouter_conv2d_dgrad_tile_ok(B, H, W, Ci, Co, kh, kw, s, p, g, tile, epi);
                            yes += scouter_conv2d_fwd_x3_tile_ok(B, H, W, Ci, Co, kh, kw, s, p, g, tile, epi);
                            yes += scouter_conv2d_dgrad_x3_tile_ok(B, H, W, Ci, Co, kh, kw, s, p, g, tile, epi);
                            calls += 4;
                            for (int io = 0; io < 32; io += 3)
                                for (int rr = 0; rr < 2; ++rr) {
                                    yes += scouter_conv2d_fwd_bf16_tile_ok(B, H, W, Ci, Co, kh, kw, s, p, g, tile, epi, io & 3, rr);
                                    yes += scouter_conv2d_dgrad_bf16_tile_ok(B, H, W, Ci, Co, kh, kw, s, p, g, tile, epi, io, rr);
                                    calls += 2;
                                }
                            for (int np = 1; np <= 3; np += 2) {
                                yes += scouter_conv2d_fwd_planes_tile_ok(B, H, W, Ci, Co, kh, kw, s, p, g, np, tile, epi, epi & 2);
                                yes += scouter_conv2d_dgrad_planes_tile_ok(B, H, W, Ci, Co, kh, kw, s, p, g, np, tile, epi);
                                calls += 2;
                            }
                        }
                    for (int k = 0; k <= 5; ++k, ++calls) yes += scouter_conv2d_wgrad_kernel_ok(B, H, W, Ci, Co, kh, kw, s, p, g, k);
                    for (int plan : {-1, 0, 3, 51})
                        for (int k = 0; k <= 1; ++k)
                            for (int field = 0; field <= 4; ++field, ++calls)
                                yes += scouter_conv2d_wgrad_plan(B, H, W, Ci, Co, kh, kw, s, p, g, k, plan, field) >= 0;
                    for (int plan : {-1, 0, 3, 51, 64, 67})
                        for (int np = 1; np <= 3; np += 2, ++calls)
                            yes += scouter_conv2d_wgrad_planes_plan_ok(B, H, W, Ci, Co, kh, kw, p, g, np, plan);
                    yes += scouter_conv2d_wgrad_x3_ok(B, H, W, Ci, Co);
                    const long pixels = (double)B * H * W < 9e18 ? (long)B * H * W : 0x7fffffffffffffffL;
                    for (int tile = 0; tile <= 6; ++tile, ++calls) yes += scouter_conv2d_planes_partial_rows(pixels, tile) > 0;
                    ++calls;
                }
    printf("route queries: %ld calls, %ld accepted, no undefined behaviour reported\n", calls, yes);
    return 0;
}
