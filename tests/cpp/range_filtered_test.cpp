// The C++ shim's filtered range search (include/hnsw_amd/graph.hpp Graph<K>::RangeSearch with
// a Filter) over the C ABI.  Compiled by tests/test_cpp_range_filtered.py and run there on the
// GPU.  Exit code = failures.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "hnsw_amd/graph.hpp"

static int failures = 0;
#define REQUIRE(cond, name)                                              \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s: %s (line %d)\n", name, #cond, __LINE__); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// 600 points on a line, the even ones allowed: the hits of a radius are the even keys of an interval
static void TestFilteredRangeSearch() {
    using G = hnsw::Graph<int>;
    G g(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    for (int i = 0; i < 600; ++i) REQUIRE(!g.Add(hnsw::MakeNode(i, {(float)i})), "add");
    std::vector<int> even;
    for (int i = 0; i < 600; i += 2) even.push_back(i);
    G::Filter f = g.MakeFilter(even);  // 300 rows: the fused path
    REQUIRE(!f.Err(), "filter");
    auto r = g.RangeSearch({64.0f}, 4.0f, &f);  // inclusive: 60 and 68 sit on the radius
    REQUIRE(!r.second && r.first.size() == 5, "len");
    if (r.first.size() == 5) {
        REQUIRE(r.first[0].node.Key == 64 && r.first[1].node.Key == 62 && r.first[2].node.Key == 66 &&
                    r.first[3].node.Key == 60 && r.first[4].node.Key == 68,
                "keys by (distance, row)");
        REQUIRE(r.first[0].Distance == 0.f && r.first[2].Distance == 2.f && r.first[4].Distance == 4.f, "distances");
        REQUIRE(r.first[3].node.Value.size() == 1 && r.first[3].node.Value[0] == 60.f, "values");
    }
    r = g.RangeSearch({64.0f}, std::nextafter(4.0f, 0.f), &f);
    REQUIRE(!r.second && r.first.size() == 3, "below the boundary");
    r = g.RangeSearch({65.0f}, 0.5f, &f);
    REQUIRE(!r.second && r.first.empty(), "the nearest row is not allowed");
    r = g.RangeSearch({64.0f}, 1000.f, &f);
    REQUIRE(!r.second && r.first.size() == 300 && r.first[299].node.Key == 598, "every allowed row");
    r = g.RangeSearch({64.0f}, -1.f, &f);
    REQUIRE(!r.second && r.first.empty(), "negative radius");
    // no filter: the plain call
    auto p = g.RangeSearch({64.0f}, 2.0f, (const G::Filter*)nullptr);
    auto q = g.RangeSearch({64.0f}, 2.0f);
    REQUIRE(!p.second && !q.second && p.first.size() == 5 && q.first.size() == 5, "nullptr is every live row");
    // a deleted allowed row is never a hit
    REQUIRE(g.Delete(62), "delete");
    r = g.RangeSearch({64.0f}, 2.0f, &f);
    REQUIRE(!r.second && r.first.size() == 2 && r.first[1].node.Key == 66, "after delete");
    // a small filter (below one row tile: the sweep over the id list) and an empty one
    G::Filter few = g.MakeFilter({10, 62, 70, 599});
    r = g.RangeSearch({64.0f}, 54.0f, &few);
    REQUIRE(!r.second && r.first.size() == 2 && r.first[0].node.Key == 70 && r.first[1].node.Key == 10, "small filter");
    G::Filter none = g.MakeFilter({});
    r = g.RangeSearch({64.0f}, 1000.f, &none);
    REQUIRE(!r.second && r.first.empty(), "empty filter");
    // beam mode: the hits the filtered walk finds, a subset of the exact ones
    auto b = g.RangeSearch({64.0f}, 6.0f, &f, MHNSW_MODE_BEAM, 32, 256);
    auto x = g.RangeSearch({64.0f}, 6.0f, &f);
    REQUIRE(!b.second && !x.second && x.first.size() == 6 && b.first.size() <= x.first.size(), "beam");
    for (const auto& hit : b.first) REQUIRE(hit.Distance <= 6.0f && hit.node.Key % 2 == 0 && hit.node.Key != 62, "beam hits");
    // errors
    auto e = g.RangeSearch({64.0f}, 1.0f, &f, MHNSW_MODE_COMPAT);
    REQUIRE(e.second.code == MHNSW_EUNSUPPORTED && e.second.msg == "range search supports beam and exact mode", "compat");
    e = g.RangeSearch({64.0f}, 1.0f, &f, MHNSW_MODE_BEAM, 129);
    REQUIRE(e.second.code == MHNSW_EUNSUPPORTED && e.second.msg == "filtered search supports max(ef,k) <= 128", "ef");
    e = g.RangeSearch({1.f, 2.f}, 1.0f, &f);
    REQUIRE(e.second.code == MHNSW_EDIM, "dim");
    G other(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    REQUIRE(!other.Add(hnsw::MakeNode(1, {1.f})), "add");
    e = other.RangeSearch({1.f}, 1.0f, &f);
    REQUIRE(e.second.code == MHNSW_EINVAL && e.second.msg == "filter of another graph", "owner");
    few.Close();
    e = g.RangeSearch({64.0f}, 1.0f, &few);
    REQUIRE(e.second.code == MHNSW_EINVAL && e.second.msg == "unknown filter -1", "closed");
}

int main() {
    TestFilteredRangeSearch();
    if (failures == 0) std::printf("PASS\n");
    return failures;
}
