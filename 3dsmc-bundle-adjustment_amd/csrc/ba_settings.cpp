// ba_settings.cpp — the table of ba_prepare's MIBA_* settings (ba_settings.h).
#include "ba_settings.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace miba {
namespace {

struct Row {
    const char* name;
    bool keyed;                              // part of the plan-cache key
    void (*parse)(Settings&, const char*);   // called when the variable is set (v is never null)
};

bool is0(const char* v) { return v[0] == '0'; }
bool is1(const char* v) { return v[0] == '1'; }

const Row kTable[] = {
    {"MIBA_OBS32", true, [](Settings& s, const char* v) { s.obs32 = !is0(v); }},
    {"MIBA_TILE_PTS", true, [](Settings& s, const char* v) { s.tile_pts = std::max(1, std::atoi(v)); }},
    {"MIBA_SUBSEG", true, [](Settings& s, const char* v) { s.subseg = std::max(64, std::atoi(v)); }},
    {"MIBA_SOLVER", true, [](Settings& s, const char* v) {
         s.solver = !std::strcmp(v, "dense") ? 0 : !std::strcmp(v, "band") ? 1 : !std::strcmp(v, "bcr") ? 2
                    : !std::strcmp(v, "blocked") ? 3 : -1;
     }},
    {"MIBA_DENSE_CHOL", true, [](Settings& s, const char* v) { s.dense_chol = is1(v); }},
    {"MIBA_BCR", true, [](Settings& s, const char* v) {
         s.bcr_set = true;
         s.bcr = !std::strcmp(v, "launch") ? 0 : !std::strcmp(v, "persist") ? 1 : !std::strcmp(v, "split") ? 2 : -1;
     }},
    {"MIBA_XCD_MAP", true, [](Settings& s, const char* v) { s.xcd_map = !is0(v); }},
    {"MIBA_FUSED", true, [](Settings& s, const char* v) { s.fused = !is0(v); }},
    {"MIBA_SW", true, [](Settings& s, const char* v) { s.sw = is0(v) ? 0 : v[0] == '2' ? 2 : 1; }},
    {"MIBA_FPL", true, [](Settings& s, const char* v) { s.fpl = is1(v); }},
    {"MIBA_BCR_DENSE1", true, [](Settings& s, const char* v) { s.bcr_dense1 = !is0(v); }},
    {"MIBA_PP_LANES", true, [](Settings& s, const char* v) {
         const int l = std::atoi(v);
         if (l == 1 || l == 2 || l == 4) s.pp_lanes = l;
     }},
    {"MIBA_DEVICE_PLAN", true, [](Settings& s, const char* v) { s.device_plan = is0(v) ? 0 : is1(v) ? 1 : -1; }},
    {"MIBA_TAIL", true, [](Settings& s, const char* v) { s.tail = !is0(v); }},
    {"MIBA_BCR_BAND", true, [](Settings& s, const char* v) { s.bcr_band = std::atoi(v); }},
    {"MIBA_BCR_XMAP", true, [](Settings& s, const char* v) { s.bcr_xmap = is1(v); }},
    {"MIBA_BLOCKED_MIN", true, [](Settings& s, const char* v) {
         s.blocked_min_set = true;
         s.blocked_min = std::atoll(v);
     }},
    {"MIBA_BSFIN", true, [](Settings& s, const char* v) { s.bsfin = is1(v); }},
    {"MIBA_VALUE_CHUNKS", false, [](Settings& s, const char* v) { s.value_chunks = std::max(1, std::min(64, std::atoi(v))); }},
    {"MIBA_MATCH_SLICES", false, [](Settings& s, const char* v) { s.match_slices = std::max(0, std::atoi(v)); }},
    {"MIBA_PLAN_TIMES", false, [](Settings& s, const char*) { s.plan_times = true; }},
    {"MIBA_PREP_TIMES", false, [](Settings& s, const char*) { s.prep_times = true; }},
};

}  // namespace

Settings read_settings() {
    Settings s;
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&h](const char* t) {
        for (; *t; ++t) h = (h ^ (unsigned char)*t) * 1099511628211ull;
    };
    for (const Row& r : kTable) {
        const char* v = std::getenv(r.name);
        if (v) r.parse(s, v);
        if (!r.keyed) continue;
        mix(r.name);
        mix(v ? "=" : "\x01");  // unset differs from set to the empty string
        if (v) mix(v);
    }
    s.key = h;
    return s;
}

}  // namespace miba
