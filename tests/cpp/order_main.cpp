// order_main — the camera ordering of ba_order.cpp as a stand-alone program (test_order_host.py).
// Reads a binary file: int32 n_cams, int32 fixed_cam, int32 W[n_cams * n_cams]. Prints
//   n_active n_edges n_components band_before band_after
//   order[0] .. order[n_cams - 1]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ba_order.h"

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: order_main weights.bin\n"); return 2; }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int32_t hdr[2];
    if (std::fread(hdr, sizeof(int32_t), 2, f) != 2 || hdr[0] < 0) { std::fprintf(stderr, "bad header\n"); return 2; }
    const size_t n = (size_t)hdr[0];
    std::vector<int32_t> W(n * n + 1);
    if (std::fread(W.data(), sizeof(int32_t), n * n, f) != n * n) { std::fprintf(stderr, "short read\n"); return 2; }
    std::fclose(f);
    miba::CamOrder co;
    miba::covis_order(W.data(), hdr[0], hdr[1], co);
    std::printf("%d %d %d %d %d\n", co.n_active, co.n_edges, co.n_components, co.band_before, co.band_after);
    for (size_t k = 0; k < co.order.size(); ++k) std::printf("%d%c", co.order[k], k + 1 < co.order.size() ? ' ' : '\n');
    if (co.order.empty()) std::printf("\n");
    return 0;
}
