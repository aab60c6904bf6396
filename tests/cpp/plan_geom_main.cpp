// plan_geom_main.cpp — prints the host plan of a window given in a file (built by tests/test_plan_geometry.py).
//
// Links only csrc/ba_plan.cpp. The file (written by the test, native byte order) holds
//   int32  nc, np, no, fixed_cam, n_params
//   int32  n_params x { tile_win, chunk_pts, chunk_obs, tile_slots, tile_pts_env, bs_pts, bs_obs, subseg }
//   int32  obs_cam[no], obs_pt[no]
//   double obs_depth[no]
// and the harness prints, per PlanParams, a line "--- k" and then one line per plan array: its name and its values.
// The arrays themselves, not hashes: the test compares them with a restatement of the geometry (tests/refschur.py)
// and checks the invariants of the Schur tiles, chunks and sub-segments on them.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ba_plan.h"

using miba::Plan;
using miba::PlanInput;
using miba::PlanParams;

template <class T>
static bool read_n(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

static void emit(const char* name, const std::vector<int>& v) {
    std::printf("%s", name);
    for (int x : v) std::printf(" %d", x);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: plan_geom_main <window file>\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "plan_geom_main: cannot open %s\n", argv[1]);
        return 2;
    }
    std::vector<int32_t> hdr, prm, oc, op;
    std::vector<double> depth;
    bool ok = read_n(f, hdr, 5) && hdr[0] >= 0 && hdr[1] >= 0 && hdr[2] >= 0 && hdr[4] >= 0 && hdr[4] <= 64;
    ok = ok && read_n(f, prm, 8 * (size_t)hdr[4]);
    ok = ok && read_n(f, oc, (size_t)hdr[2]) && read_n(f, op, (size_t)hdr[2]) && read_n(f, depth, (size_t)hdr[2]);
    std::fclose(f);
    if (!ok) {
        std::fprintf(stderr, "plan_geom_main: short or malformed file\n");
        return 2;
    }
    PlanInput in;
    in.nc = hdr[0];
    in.np = hdr[1];
    in.no = hdr[2];
    in.fixed_cam = hdr[3];
    in.obs_cam = oc.data();
    in.obs_pt = op.data();
    in.obs_depth = depth.data();
    for (int k = 0; k < hdr[4]; ++k) {
        const int32_t* q = prm.data() + 8 * k;
        PlanParams pp;
        pp.tile_win = q[0];
        pp.chunk_pts = q[1];
        pp.chunk_obs = q[2];
        pp.tile_slots = q[3];
        pp.tile_pts_env = q[4];
        pp.bs_pts = q[5];
        pp.bs_obs = q[6];
        pp.subseg = q[7];
        Plan pl;
        miba::plan_count(in, pl);
        std::printf("--- %d\n", k);
        if (!pl.err.empty()) {
            std::printf("err %s\n", pl.err.c_str());
            continue;
        }
        std::vector<int> cam_seen(in.nc);
        for (int i = 0; i < in.nc; ++i) cam_seen[i] = pl.cam_cnt[i] > 0;
        miba::plan_order(in, cam_seen, pp, pl);
        miba::plan_envelope(pl);
        emit("scalars", {pl.n_adm, pl.nac, pl.n_ap(), pl.n_tiled, pl.n_ovf()});
        emit("cam_cnt", pl.cam_cnt); emit("pt_cnt", pl.pt_cnt); emit("cam_ac", pl.cam_ac); emit("ac_cam", pl.ac_cam);
        emit("pmin", pl.pmin); emit("pmax", pl.pmax); emit("pt_idx", pl.pt_idx); emit("pt_ptr", pl.pt_ptr);
        emit("po_orig", pl.po_orig); emit("co_orig", pl.co_orig);
        emit("tile_chunk", pl.tile_chunk); emit("tile_base", pl.tile_base); emit("tile_span", pl.tile_span);
        emit("chunk_ap", pl.chunk_ap); emit("ovf_obs", pl.ovf_obs); emit("bs_chunk", pl.bs_chunk);
        emit("seg_ptr", pl.seg_ptr); emit("seg_cam", pl.seg_cam); emit("seg_ac", pl.seg_ac); emit("ac_seg", pl.ac_seg);
        emit("fc", pl.fc);
    }
    std::printf("plan_geom_main: ok\n");
    return 0;
}
