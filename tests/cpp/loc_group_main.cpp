// loc_group_main.cpp — prints ba_localize's grouping of a window's observations by camera (built by
// tests/test_loc_group.py).
//
// Links only csrc/ba_loc_group.cpp. The file (written by the test, native byte order) holds
//   int32  nc, no, has_mask
//   int32  obs_cam[no]
//   double obs_depth[no]
//   uint8  mask[nc]          (when has_mask)
// and the harness prints three lines: "kept n", "off ..." (nc + 1 values) and "idx ..." (n values).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ba_loc_group.h"

template <class T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: loc_group_main <window file>\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "loc_group_main: cannot open %s\n", argv[1]);
        return 2;
    }
    int32_t hdr[3];
    std::vector<int32_t> cam;
    std::vector<double> dep;
    std::vector<uint8_t> mask;
    bool ok = std::fread(hdr, sizeof(int32_t), 3, f) == 3 && hdr[0] >= 0 && hdr[1] >= 0;
    ok = ok && read_n(f, cam, (size_t)hdr[1]) && read_n(f, dep, (size_t)hdr[1]);
    if (ok && hdr[2]) ok = read_n(f, mask, (size_t)hdr[0]);
    std::fclose(f);
    if (!ok) {
        std::fprintf(stderr, "loc_group_main: short file\n");
        return 2;
    }
    std::vector<int32_t> off((size_t)hdr[0] + 1, -1), idx((size_t)hdr[1] + 1, -1);
    const int32_t n = miba::loc_group(hdr[0], hdr[1], cam.data(), dep.data(), hdr[2] ? mask.data() : nullptr, off.data(),
                                      idx.data());
    std::printf("kept %d\noff", n);
    for (int32_t x : off) std::printf(" %d", x);
    std::printf("\nidx");
    for (int32_t k = 0; k < n; ++k) std::printf(" %d", idx[(size_t)k]);
    std::printf("\n");
    return idx[(size_t)hdr[1]] == -1 ? 0 : 3;  // nothing written past n_obs entries
}
