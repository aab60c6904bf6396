// ba_order.cpp — reverse Cuthill-McKee ordering of a window's cameras from the co-visibility weights (ba_order.h).
// Host code only: the graph has one node per camera, a few thousand at most.
#include "ba_order.h"

#include <algorithm>

namespace miba {

int covis_band(const int32_t* W, int n_cams, const int32_t* order, int n_active) {
    int band = 0;
    for (int a = 0; a < n_active; ++a) {
        const int32_t* row = W + (size_t)order[a] * n_cams;
        int fc = a;
        for (int b = 0; b < a; ++b)
            if (row[order[b]] > 0) { fc = b; break; }
        band = std::max(band, a - fc);
    }
    return band;
}

void covis_order(const int32_t* W, int n_cams, int fixed_cam, CamOrder& out) {
    covis_order(W, n_cams, fixed_cam, nullptr, out);
}

void covis_order(const int32_t* W, int n_cams, int fixed_cam, const uint8_t* cam_const, CamOrder& out) {
    const int n = n_cams;
    out = CamOrder{};
    std::vector<char> act(n, 0);
    std::vector<int32_t> given;  // the active cameras as given
    for (int i = 0; i < n; ++i)
        if (W[(size_t)i * n + i] > 0 && i != fixed_cam && !(cam_const && cam_const[i])) { act[i] = 1; given.push_back(i); }
    out.n_active = (int)given.size();
    std::vector<int> deg(n, 0);
    for (int i : given) {
        const int32_t* row = W + (size_t)i * n;
        for (int j : given)
            if (j != i && row[j] > 0) ++deg[i];
        out.n_edges += deg[i];
    }
    out.n_edges /= 2;
    const auto by_degree = [&](int a, int b) { return deg[a] != deg[b] ? deg[a] < deg[b] : a < b; };
    std::vector<int32_t> starts(given);  // by (degree, index): the first unvisited one starts the next component
    std::sort(starts.begin(), starts.end(), by_degree);
    std::vector<char> visited(n, 0);
    out.order.reserve(n);
    std::vector<int32_t> nb;
    for (int s : starts) {
        if (visited[s]) continue;
        ++out.n_components;
        const size_t first = out.order.size();
        out.order.push_back(s);
        visited[s] = 1;
        for (size_t head = first; head < out.order.size(); ++head) {
            const int32_t* row = W + (size_t)out.order[head] * n;
            nb.clear();
            for (int j : given)
                if (!visited[j] && row[j] > 0) nb.push_back(j);
            std::sort(nb.begin(), nb.end(), by_degree);
            for (int j : nb) { visited[j] = 1; out.order.push_back(j); }
        }
        std::reverse(out.order.begin() + first, out.order.end());
    }
    for (int i = 0; i < n; ++i)
        if (!act[i]) out.order.push_back(i);
    out.band_before = covis_band(W, n, given.data(), out.n_active);
    out.band_after = covis_band(W, n, out.order.data(), out.n_active);
}

}  // namespace miba
