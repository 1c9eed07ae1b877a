// The C++ shim's range search (include/hnsw_amd/graph.hpp Graph<K>::RangeSearch) over the C
// ABI.  Compiled by tests/test_cpp_range.py and run there on the GPU.  Exit code = failures.
#include <cmath>
#include <cstdio>
#include <string>

#include "hnsw_amd/graph.hpp"

static int failures = 0;
#define REQUIRE(cond, name)                                              \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAIL %s: %s (line %d)\n", name, #cond, __LINE__); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// 300 points on a line: the hits of a radius are an interval
static void TestRangeSearch() {
    hnsw::Graph<int> g(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    for (int i = 0; i < 300; ++i) REQUIRE(!g.Add(hnsw::MakeNode(i, {(float)i})), "add");
    auto r = g.RangeSearch({64.0f}, 2.0f);  // inclusive: 62 and 66 sit on the radius
    REQUIRE(!r.second && r.first.size() == 5, "len");
    if (r.first.size() == 5) {
        REQUIRE(r.first[0].node.Key == 64 && r.first[1].node.Key == 63 && r.first[2].node.Key == 65 &&
                    r.first[3].node.Key == 62 && r.first[4].node.Key == 66,
                "keys by (distance, row)");
        REQUIRE(r.first[0].Distance == 0.f && r.first[2].Distance == 1.f && r.first[4].Distance == 2.f, "distances");
        REQUIRE(r.first[3].node.Value.size() == 1 && r.first[3].node.Value[0] == 62.f, "values");
    }
    r = g.RangeSearch({64.0f}, std::nextafter(2.0f, 0.f));
    REQUIRE(!r.second && r.first.size() == 3, "below the boundary");
    r = g.RangeSearch({64.4f}, 0.25f);
    REQUIRE(!r.second && r.first.empty(), "no hit");
    r = g.RangeSearch({64.0f}, 1000.f);  // more than any top-k list holds
    REQUIRE(!r.second && r.first.size() == 300 && r.first[299].node.Key == 299, "every row");
    r = g.RangeSearch({64.0f}, -1.f);
    REQUIRE(!r.second && r.first.empty(), "negative radius");
    r = g.RangeSearch({64.0f}, std::nanf(""));
    REQUIRE(!r.second && r.first.empty(), "NaN radius");
    // a deleted row is never a hit
    REQUIRE(g.Delete(63), "delete");
    r = g.RangeSearch({64.0f}, 1.0f);
    REQUIRE(!r.second && r.first.size() == 2 && r.first[1].node.Key == 65, "after delete");
    // beam mode: the hits the beam search finds, a subset of the exact ones
    auto b = g.RangeSearch({64.0f}, 3.0f, MHNSW_MODE_BEAM, 32);
    auto x = g.RangeSearch({64.0f}, 3.0f);
    REQUIRE(!b.second && !x.second && x.first.size() == 6 && b.first.size() <= x.first.size(), "beam");
    for (const auto& hit : b.first) REQUIRE(hit.Distance <= 3.0f && hit.node.Key != 63, "beam hits");
    // errors
    auto e = g.RangeSearch({64.0f}, 1.0f, MHNSW_MODE_COMPAT);
    REQUIRE(e.second.code == MHNSW_EUNSUPPORTED && e.second.msg == "range search supports beam and exact mode", "compat");
    e = g.RangeSearch({1.f, 2.f}, 1.0f);
    REQUIRE(e.second.code == MHNSW_EDIM, "dim");
    // string keys
    hnsw::Graph<std::string> s(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    for (int i = 0; i < 40; ++i) REQUIRE(!s.Add(hnsw::MakeNode(std::string("k") + std::to_string(100 + i), {(float)i})), "add");
    auto sr = s.RangeSearch({7.0f}, 1.0f);
    REQUIRE(!sr.second && sr.first.size() == 3 && sr.first[0].node.Key == "k107" && sr.first[1].node.Key == "k106" &&
                sr.first[2].node.Key == "k108",
            "string keys");
}

int main() {
    TestRangeSearch();
    if (failures == 0) std::printf("PASS\n");
    return failures;
}
