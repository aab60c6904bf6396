// plan_mask_main.cpp — prints the host plan of a window under a set of constant cameras (tests/test_plan_mask.py).
//
// Links only csrc/ba_plan.cpp. The file (written by the test, native byte order) holds
//   int32  nc, np, no, fixed_cam, has_mask
//   uint8  mask[nc]                 (has_mask != 0)
//   int32  obs_cam[no], obs_pt[no]
//   double obs_depth[no]
// The plan is built with PlanParams' defaults and PlanInput::cam_const = the mask (nullptr without one); the harness
// prints one line per plan array: its name and its values.
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
        std::fprintf(stderr, "usage: plan_mask_main <window file>\n");
        return 2;
    }
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) {
        std::fprintf(stderr, "plan_mask_main: cannot open %s\n", argv[1]);
        return 2;
    }
    std::vector<int32_t> hdr, oc, op;
    std::vector<uint8_t> mask;
    std::vector<double> depth;
    bool ok = read_n(f, hdr, 5) && hdr[0] >= 0 && hdr[1] >= 0 && hdr[2] >= 0;
    ok = ok && (!hdr[4] || read_n(f, mask, (size_t)hdr[0]));
    ok = ok && read_n(f, oc, (size_t)hdr[2]) && read_n(f, op, (size_t)hdr[2]) && read_n(f, depth, (size_t)hdr[2]);
    std::fclose(f);
    if (!ok) {
        std::fprintf(stderr, "plan_mask_main: short or malformed file\n");
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
    if (hdr[4]) in.cam_const = mask.data();
    Plan pl;
    miba::plan_count(in, pl);
    if (!pl.err.empty()) {
        std::printf("err %s\n", pl.err.c_str());
        return 1;
    }
    std::vector<int> cam_seen(in.nc);
    for (int i = 0; i < in.nc; ++i) cam_seen[i] = pl.cam_cnt[i] > 0;
    miba::plan_order(in, cam_seen, PlanParams{}, pl);
    miba::plan_envelope(pl);
    emit("scalars", {pl.n_adm, pl.nac, pl.n_ap(), pl.n_tiled, pl.n_ovf(), pl.n, pl.cam_band, pl.band_w});
    emit("cam_cnt", pl.cam_cnt); emit("pt_cnt", pl.pt_cnt); emit("cam_ac", pl.cam_ac); emit("ac_cam", pl.ac_cam);
    emit("pmin", pl.pmin); emit("pmax", pl.pmax); emit("pt_idx", pl.pt_idx); emit("pt_ptr", pl.pt_ptr);
    emit("po_orig", pl.po_orig); emit("co_orig", pl.co_orig); emit("po_dest", pl.po_dest); emit("co_dest", pl.co_dest);
    emit("tile_chunk", pl.tile_chunk); emit("tile_base", pl.tile_base); emit("tile_span", pl.tile_span);
    emit("chunk_ap", pl.chunk_ap); emit("ovf_obs", pl.ovf_obs); emit("bs_chunk", pl.bs_chunk);
    emit("seg_ptr", pl.seg_ptr); emit("seg_cam", pl.seg_cam); emit("seg_ac", pl.seg_ac); emit("ac_seg", pl.ac_seg);
    emit("fc", pl.fc); emit("fcol", pl.fcol); emit("rptr", pl.rptr); emit("rows", pl.rows); emit("env_tile", pl.env_tile);
    std::printf("plan_mask_main: ok\n");
    return 0;
}
