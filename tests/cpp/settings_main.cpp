// settings_main — prints what read_settings() (csrc/ba_settings.cpp) makes of the environment it is started in: one
// "field=value" line per field of miba::Settings, the plan-cache key last. tests/test_settings.py starts it with
// different environments; built from ba_settings.cpp alone (host-only), also under ASan + UBSan.
#include <cstdio>

#include "ba_settings.h"

int main() {
    // twice: equal environments give equal keys, and nothing is cached between two reads
    const miba::Settings s = miba::read_settings(), again = miba::read_settings();
    if (s.key != again.key) {
        std::fprintf(stderr, "settings_main: two reads of one environment gave different keys\n");
        return 1;
    }
    std::printf("obs32=%d\nfused=%d\ntail=%d\nxcd_map=%d\nbcr_dense1=%d\n", s.obs32, s.fused, s.tail, s.xcd_map,
                s.bcr_dense1);
    std::printf("device_plan=%d\nsw=%d\n", s.device_plan, s.sw);
    std::printf("fpl=%d\nbsfin=%d\nbcr_xmap=%d\ndense_chol=%d\n", s.fpl, s.bsfin, s.bcr_xmap, s.dense_chol);
    std::printf("solver=%d\nbcr_set=%d\nbcr=%d\nbcr_band=%d\n", s.solver, s.bcr_set, s.bcr, s.bcr_band);
    std::printf("tile_pts=%d\nsubseg=%d\nblocked_min_set=%d\nblocked_min=%lld\n", s.tile_pts, s.subseg, s.blocked_min_set,
                s.blocked_min);
    std::printf("value_chunks=%d\npp_lanes=%d\nplan_times=%d\nprep_times=%d\n", s.value_chunks, s.pp_lanes, s.plan_times,
                s.prep_times);
    std::printf("key=%llu\n", s.key);
    return 0;
}
