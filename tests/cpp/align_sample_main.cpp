// Host harness of ba_align's shared device / host headers (tests/test_align_sample.py).
//   align_sample_main sample   reads "seed j h n" per line, prints the three indices of csrc/ba_align_sample.h
//   align_sample_main fit      reads min_cross and 18 hex-float coordinates per line (cloud 1's three sample points,
//                              then cloud 2's), prints "ok qx qy qz qw tx ty tz" of csrc/ba_align_fit.h as hex floats
//   align_sample_main dist2    reads a pose (7) and one correspondence (6), prints align_dist2 as a hex float
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "ba_align_fit.h"

using namespace miba;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (!std::strcmp(argv[1], "sample")) {
        uint64_t seed;
        uint32_t j, h, n;
        while (std::scanf("%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu32, &seed, &j, &h, &n) == 4) {
            uint32_t idx[3];
            align_sample(seed, j, h, n, idx);
            std::printf("%" PRIu32 " %" PRIu32 " %" PRIu32 "\n", idx[0], idx[1], idx[2]);
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "fit")) {
        double mc, a[3][3], b[3][3];
        for (;;) {
            if (std::scanf("%la", &mc) != 1) break;
            for (int i = 0; i < 3; ++i)
                for (int k = 0; k < 3; ++k)
                    if (std::scanf("%la", &a[i][k]) != 1) return 3;
            for (int i = 0; i < 3; ++i)
                for (int k = 0; k < 3; ++k)
                    if (std::scanf("%la", &b[i][k]) != 1) return 3;
            AlignModel m{};
            const bool ok = align_fit3(a, b, mc * mc, m);
            std::printf("%d %a %a %a %a %a %a %a\n", ok ? 1 : 0, m.q[0], m.q[1], m.q[2], m.q[3], m.t[0], m.t[1], m.t[2]);
        }
        return 0;
    }
    if (!std::strcmp(argv[1], "dist2")) {
        double v[13];
        for (;;) {
            for (int i = 0; i < 13; ++i)
                if (std::scanf("%la", &v[i]) != 1) return 0;
            // the model from the pose: R of the unit quaternion (x, y, z, w), as align_fit_H forms it
            AlignModel m{};
            const double x = v[0], y = v[1], z = v[2], w = v[3];
            m.R[0] = 1.0 - 2.0 * (y * y + z * z); m.R[1] = 2.0 * (x * y - z * w); m.R[2] = 2.0 * (x * z + y * w);
            m.R[3] = 2.0 * (x * y + z * w); m.R[4] = 1.0 - 2.0 * (x * x + z * z); m.R[5] = 2.0 * (y * z - x * w);
            m.R[6] = 2.0 * (x * z - y * w); m.R[7] = 2.0 * (y * z + x * w); m.R[8] = 1.0 - 2.0 * (x * x + y * y);
            m.t[0] = v[4]; m.t[1] = v[5]; m.t[2] = v[6];
            std::printf("%a\n", align_dist2(m, v[7], v[8], v[9], v[10], v[11], v[12]));
        }
    }
    return 2;
}
