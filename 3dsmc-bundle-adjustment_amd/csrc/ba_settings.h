// ba_settings.h — the MIBA_* environment settings ba_prepare reads (libmiba, internal; host-only C++).
//
// One table (ba_settings.cpp) lists every prepare-time variable: its name, how it parses and whether it is part
// of the plan-cache key. read_settings() walks that table once per prepare, before the plan-cache comparison, and
// fills the struct and the key in the same pass: a variable cannot be parsed without the table knowing whether it
// is keyed. Never cached per process (tests change the environment between two solves of one context).
//
// Read elsewhere, per solve / launch / process: MIBA_BCR_SPIN_LIMIT, MIBA_BCR_COOP, MIBA_BCR_STAMPS,
// MIBA_DUMMY_LAUNCHES, MIBA_HOST_THREADS, MIBA_DUMP_DIR, MIBA_LIB_PATH (and MIBA_PP_LANES' launch-side cache).
#pragma once

namespace miba {

struct Settings {
    // off iff the first character is '0'
    bool obs32 = true, fused = true, tail = true, xcd_map = true, bcr_dense1 = true;
    int device_plan = -1;  // MIBA_DEVICE_PLAN: 0 the host plan, 1 the device plan whenever it fits, -1 the size rule
    int sw = 1;            // MIBA_SW: 0 off, 2 every window that fits, 1 the default
    // on iff the first character is '1'
    bool fpl = false, bsfin = false, bcr_xmap = false, dense_chol = false;
    int solver = -1;       // MIBA_SOLVER: DevProblem::solver (0 dense, 1 band, 2 bcr, 3 blocked), -1 none / unknown
    bool bcr_set = false;  // MIBA_BCR is set, whatever its value: no dense1, no band path
    int bcr = -1;          // MIBA_BCR: BcrWork::persist override (0 launch, 1 persist, 2 split), -1 none
    int bcr_band = 1;      // MIBA_BCR_BAND: 0 off, 2 also one-block windows, else the default
    int tile_pts = 0;      // MIBA_TILE_PTS (>= 1), 0 unset
    int subseg = 0;        // MIBA_SUBSEG (>= 64), 0 unset
    bool blocked_min_set = false;
    long long blocked_min = 0;  // MIBA_BLOCKED_MIN when set
    int value_chunks = 0;  // MIBA_VALUE_CHUNKS (1..64), 0 unset; not keyed
    // MIBA_MATCH_SLICES (>= 1): ba_match's train slices per query tile, 0 unset; not keyed (ba_match reads the table
    // at every call: it has no prepare)
    int match_slices = 0;
    int pp_lanes = 1;      // MIBA_PP_LANES: 1 / 2 / 4 (the launches read their own per-process copy)
    bool plan_times = false, prep_times = false;  // diagnostics on stderr (set at all); not keyed
    unsigned long long key = 0;  // FNV-1a over name and value ("unset" and "" differ) of every keyed variable
};

Settings read_settings();

}  // namespace miba
