// gmatch_host_main.cpp — a stand-alone program over csrc/ba_gmatch_host.h (tests/test_gmatch_abi.py builds it with g++,
// plain and with -fsanitize=address,undefined, and runs it): the order and the texts of ba_guided_match's own
// refusals, the de-duplication of equal keypoint ranges, the default cell, the launch limits, and the cell rectangle
// of a window against a brute-force check that it covers every keypoint the exact test admits. Prints "ok <what>"
// lines and exits 0, or the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "ba_gmatch_host.h"

using namespace miba;

static int fails = 0;
static void expect(bool ok, const std::string& what) {
    if (!ok) {
        std::printf("FAILED %s\n", what.c_str());
        ++fails;
    }
}

// A small valid call; every test spoils a copy of it.
struct Call {
    std::vector<double> uv = std::vector<double>(12, 1.0), pts = std::vector<double>(9, 1.0), pose = std::vector<double>(14, 0.0);
    std::vector<uint8_t> kd = std::vector<uint8_t>(6 * 32), pd = std::vector<uint8_t>(3 * 32), status = std::vector<uint8_t>(4);
    std::vector<int32_t> range = {0, 6, 2, 5}, cbegin = {0, 3, 4}, cpt = {0, 1, 2, 1}, nn = std::vector<int32_t>(8),
                         dist = std::vector<int32_t>(8), mb = std::vector<int32_t>(3), m = std::vector<int32_t>(8);
    ba_gmatch_problem p{};
    ba_gmatch_request r{};
    Call() {
        p.kind = BA_MATCH_HAMMING; p.desc_bytes = 32; p.width = 100; p.height = 75;
        p.n_kp = 6; p.n_points = 3; p.n_frames = 2; p.n_rows = 4;
        p.kp_uv = uv.data(); p.kp_desc = kd.data(); p.points = pts.data(); p.pt_desc = pd.data();
        p.frame_pose = pose.data(); p.frame_range = range.data(); p.cand_begin = cbegin.data(); p.cand_pt = cpt.data();
        BA_GMATCH_REQUEST_INIT(r);
        r.radius = 15.0;
        r.nn_kp = nn.data(); r.nn_dist = dist.data(); r.status = status.data(); r.matches = m.data(); r.match_begin = mb.data();
    }
    std::string check() const { return gm_check(&p, &r); }
};

static void refusals() {
    { Call c; expect(c.check().empty(), "the plain call passes: " + c.check()); }
    // each defect with a later one beside it: the earlier check of the fixed order wins
    { Call c; c.p.n_kp = -1; c.p.kind = 2; expect(c.check() == "negative sizes", "negative n_kp"); }
    { Call c; c.p.n_rows = -1; c.p.kind = 2; expect(c.check() == "negative sizes", "negative n_rows"); }
    { Call c; c.p.kind = 2; c.p.desc_bytes = 30;
      expect(c.check() == "kind = 2 is neither BA_MATCH_HAMMING nor BA_MATCH_L2_U8", "kind"); }
    for (int bad : {0, 30, 260}) {
        Call c; c.p.desc_bytes = bad; c.p.width = 0;
        expect(c.check() == "desc_bytes = " + std::to_string(bad) + " is not a multiple of 4 in [4, 256]", "desc_bytes");
    }
    { Call c; c.p.width = 0; c.r.radius = -1.0; expect(c.check() == "width = 0, height = 75: both must be positive", "width"); }
    { Call c; c.p.height = -3; expect(c.check() == "width = 100, height = -3: both must be positive", "height"); }
    for (double bad : {0.0, -2.0, std::numeric_limits<double>::infinity(), std::numeric_limits<double>::quiet_NaN()}) {
        Call c; c.r.radius = bad; c.p.frame_range = nullptr;
        expect(c.check() == "radius is not a finite positive number", "radius");
    }
    { Call c; c.p.frame_pose = nullptr; c.range[1] = 7;
      expect(c.check() == "null required buffer (frame_pose / frame_range / cand_begin)", "null frame_pose"); }
    { Call c; c.p.cand_begin = nullptr; expect(c.check() == "null required buffer (frame_pose / frame_range / cand_begin)", "null cand_begin"); }
    { Call c; c.range[1] = 7; c.cbegin[0] = 1;
      expect(c.check() == "frame 0: the keypoint range [0, 7) is reversed or leaves [0, n_kp = 6)", "range end"); }
    { Call c; c.range[2] = 5; c.range[3] = 2;
      expect(c.check() == "frame 1: the keypoint range [5, 2) is reversed or leaves [0, n_kp = 6)", "range reversed"); }
    { Call c; c.range[0] = -1; expect(c.check() == "frame 0: the keypoint range [-1, 6) is reversed or leaves [0, n_kp = 6)", "range begin"); }
    { Call c; c.cbegin[0] = 1; c.cbegin[2] = 0; expect(c.check() == "cand_begin[0] = 1 is not 0", "cand_begin[0]"); }
    { Call c; c.cbegin[1] = 5; c.p.n_rows = 9; expect(c.check() == "cand_begin decreases at frame 1", "cand_begin decreases"); }
    { Call c; c.p.n_rows = 5; c.p.cand_pt = nullptr; expect(c.check() == "n_rows = 5 is not cand_begin[n_frames] (4)", "n_rows"); }
    { Call c; c.p.cand_pt = nullptr; c.p.kp_uv = nullptr; expect(c.check() == "null required buffer (cand_pt)", "null cand_pt"); }
    { Call c; c.cpt[2] = 3; c.p.kp_uv = nullptr; expect(c.check() == "cand_pt[2] = 3 leaves [0, n_points = 3)", "cand_pt high"); }
    { Call c; c.cpt[0] = -1; expect(c.check() == "cand_pt[0] = -1 leaves [0, n_points = 3)", "cand_pt low"); }
    { Call c; c.p.kp_uv = nullptr; c.p.points = nullptr; expect(c.check() == "null required buffer (kp_uv / kp_desc)", "null kp_uv"); }
    { Call c; c.p.kp_desc = nullptr; expect(c.check() == "null required buffer (kp_uv / kp_desc)", "null kp_desc"); }
    { Call c; c.p.points = nullptr; c.r.nn_kp = nullptr; expect(c.check() == "null required buffer (points / pt_desc)", "null points"); }
    { Call c; c.p.pt_desc = nullptr; expect(c.check() == "null required buffer (points / pt_desc)", "null pt_desc"); }
    { Call c; c.r.status = nullptr; c.r.match_begin = nullptr;
      expect(c.check() == "null required buffer (nn_kp / nn_dist / status)", "null status"); }
    { Call c; c.r.nn_dist = nullptr; expect(c.check() == "null required buffer (nn_kp / nn_dist / status)", "null nn_dist"); }
    { Call c; c.r.match_begin = nullptr; expect(c.check() == "null required buffer (match_begin with matches)", "null match_begin"); }
    // what may be absent: the depths, the optional outputs; everything with n_frames = 0; empty entries
    { Call c; c.r.matches = nullptr; c.r.match_begin = nullptr; expect(c.check().empty(), "no matches asked"); }
    { Call c; c.p.n_frames = 0; c.p.n_rows = 0; c.p.frame_pose = nullptr; c.p.frame_range = nullptr; c.p.cand_begin = nullptr;
      c.p.cand_pt = nullptr; c.p.points = nullptr; c.r.nn_kp = nullptr; expect(c.check().empty(), "n_frames = 0: " + c.check()); }
    { Call c; c.cbegin = {0, 0, 0}; c.p.n_rows = 0; c.p.cand_pt = nullptr; c.p.points = nullptr; c.p.pt_desc = nullptr;
      c.r.nn_kp = nullptr; expect(c.check().empty(), "no candidates: " + c.check()); }
    std::printf("ok refusals\n");
}

static void layout_and_limits() {
    const std::vector<int32_t> fr = {0, 6, 2, 5, 0, 6, 3, 3, 2, 5, 0, 6, 0, 5};
    const GmLayout L = gm_layout(fr.data(), 7);
    expect(L.n_grids() == 4, "four distinct ranges");
    expect(L.frame_grid == std::vector<int32_t>({0, 1, 0, 2, 1, 0, 3}), "frame_grid in the order of first appearance");
    expect(L.grid_range == std::vector<int32_t>({0, 6, 2, 5, 3, 3, 0, 5}), "grid_range");
    expect(L.grid_kp_begin == std::vector<long long>({0, 6, 9, 9, 14}), "grid_kp_begin");
    expect(L.o2o_begin == std::vector<long long>({0, 6, 9, 15, 15, 18, 24, 29}), "o2o_begin stays per frame entry");
    std::vector<int32_t> same(2 * 1024);
    for (int f = 0; f < 1024; ++f) { same[2 * f] = 0; same[2 * f + 1] = 2000; }
    const GmLayout H = gm_layout(same.data(), 1024);
    expect(H.n_grids() == 1 && H.grid_kp_begin.back() == 2000 && H.o2o_begin.back() == 1024 * 2000, "1024 hypotheses bin once");
    expect(gm_layout(nullptr, 0).n_grids() == 0, "no frames");

    expect(gm_default_cell(15.0) == 16 && gm_default_cell(16.0) == 16 && gm_default_cell(16.5) == 32 &&
           gm_default_cell(3.0) == 8 && gm_default_cell(1e300) == (1 << 30), "the default cell");
    const GmGrid g = gm_grid(100, 75, 0, 15.0);
    expect(g.cell == 16 && g.gw == 7 && g.gh == 5 && g.cells() == 35, "100 x 75 at 16");
    const GmGrid one = gm_grid(100, 75, 4096, 15.0);
    expect(one.cell == 4096 && one.cells() == 1, "one cell");

    Call c;
    expect(gm_limits(&c.p, g, L).empty(), "the plain call is inside the limits");
    c.p.width = c.p.height = 2147483647;
    const GmGrid huge = gm_grid(c.p.width, c.p.height, 8, 15.0);
    expect(gm_limits(&c.p, huge, L) == "the grid of 268435456 x 268435456 cells x 4 keypoint ranges is above the limit of 2^31 - 1 cells",
           "too many cells: " + gm_limits(&c.p, huge, L));
    Call d;
    d.p.n_frames = 1 << 24;
    expect(gm_limits(&d.p, g, L) == "the grid of 16777216 frames x 256 threads is above the launch limit of 2^32 threads", "too many frames");
    GmLayout big = L;
    big.o2o_begin.back() = 1LL << 31;
    expect(gm_limits(&c.p, g, big) == "the 2147483648 one-to-one slots are above the limit of 2^31 - 1", "too many slots");
    big = L;
    big.grid_kp_begin.back() = 1LL << 31;
    expect(gm_limits(&c.p, g, big) == "the 2147483648 binned keypoints are above the limit of 2^31 - 1", "too many binned keypoints");
    std::printf("ok layout and limits\n");
}

// the window test, as the kernel evaluates it
static bool in_disc(double ku, double kv, double u, double v, double r2) {
    const volatile double du = ku - u, dv = kv - v;
    const volatile double a = du * du, b = dv * dv;
    return a + b <= r2;
}

static void superset() {
    std::mt19937_64 gen(7);
    long long admitted = 0, visited = 0, total = 0;
    for (int cell : {1, 3, 8, 16, 64, 4096}) {
        for (double radius : {0.5, 3.0, 8.0, 15.0, 16.0, 40.0, 1000.0}) {
            const int W = 100, H = 75;
            const GmGrid g = gm_grid(W, H, cell, radius);
            const double inv = 1.0 / (double)g.cell, r2 = radius * radius;
            std::uniform_real_distribution<double> pu(0.0, W), pv(0.0, H), off(-1.0, 1.0);
            for (int it = 0; it < 300; ++it) {
                // projections anywhere in the image, on cell boundaries and at the borders
                double u = pu(gen), v = pv(gen);
                if (it % 5 == 1) u = (double)(g.cell * (int)(u * inv));
                if (it % 5 == 2) v = (double)(g.cell * (int)(v * inv));
                if (it % 7 == 3) u = 0.0;
                if (it % 7 == 4) v = std::nextafter((double)H, 0.0);
                int xlo, xhi, ylo, yhi;
                gm_cell_span(u, radius, inv, g.gw, xlo, xhi);
                gm_cell_span(v, radius, inv, g.gh, ylo, yhi);
                expect(0 <= xlo && xlo <= xhi && xhi < g.gw && 0 <= ylo && ylo <= yhi && yhi < g.gh, "the span is inside the grid");
                for (int k = 0; k < 60; ++k) {
                    // keypoints on the disc's edge to within rounding, inside, outside, on cell boundaries, off the image
                    const double phi = 6.283185307179586 * (double)k / 60.0;
                    double rho = radius;
                    if (k % 4 == 1) rho = std::nextafter(radius, 0.0);
                    if (k % 4 == 2) rho = std::nextafter(radius, 2 * radius);
                    if (k % 4 == 3) rho = radius * (1.0 + off(gen));
                    double ku = u + rho * std::cos(phi), kv = v + rho * std::sin(phi);
                    if (k % 6 == 5) ku = (double)(g.cell * (int)std::floor(ku * inv));
                    if (k == 0) { ku = u + radius; kv = v; }
                    if (k == 30) { ku = u; kv = v - radius; }
                    const int cx = gm_cell_of(ku, inv, g.gw), cy = gm_cell_of(kv, inv, g.gh);
                    expect(0 <= cx && cx < g.gw && 0 <= cy && cy < g.gh, "a keypoint's cell is inside the grid");
                    const bool in = in_disc(ku, kv, u, v, r2), seen = xlo <= cx && cx <= xhi && ylo <= cy && cy <= yhi;
                    ++total;
                    admitted += in;
                    visited += seen;
                    if (in && !seen) {
                        std::printf("FAILED superset: cell %d radius %g u %.17g v %.17g ku %.17g kv %.17g\n", g.cell, radius, u, v, ku, kv);
                        ++fails;
                    }
                }
            }
        }
    }
    expect(admitted > total / 4 && visited < total, "the check saw admitted keypoints and cells left out");
    // what is not a number or far off sits in a border cell
    expect(gm_cell_of(std::numeric_limits<double>::quiet_NaN(), 0.125, 13) == 0 && gm_cell_of(-5.0, 0.125, 13) == 0 &&
           gm_cell_of(1e300, 0.125, 13) == 12 && gm_cell_of(std::numeric_limits<double>::infinity(), 0.125, 13) == 12 &&
           gm_cell_of(8.0, 0.125, 13) == 1 && gm_cell_of(std::nextafter(8.0, 0.0), 0.125, 13) == 0, "the clamp");
    std::printf("ok superset admitted=%lld visited=%lld of=%lld\n", admitted, visited, total);
}

int main() {
    refusals();
    layout_and_limits();
    superset();
    if (fails) return 1;
    std::printf("ok all\n");
    return 0;
}
