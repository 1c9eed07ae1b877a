// The C++ shim's filtered exact search (include/hnsw_amd/graph.hpp Graph<K>::SearchFilteredExact)
// over the C ABI.  Compiled by tests/test_filtered_exact_hosts.py and run there on the GPU.
// Exit code = failures.
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

// 300 points on a line; the filter allows the multiples of 4
static void TestSearchFilteredExact() {
    hnsw::Graph<int> g(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    for (int i = 0; i < 300; ++i) REQUIRE(!g.Add(hnsw::MakeNode(i, {(float)i})), "add");
    std::vector<int> fours;
    for (int i = 0; i < 300; i += 4) fours.push_back(i);
    auto f = g.MakeFilter(fours);
    REQUIRE(!f.Err(), "create");
    auto r = g.SearchFilteredExact({64.4f}, 4, &f);
    REQUIRE(!r.second && r.first.size() == 4, "len");
    if (r.first.size() == 4)
        REQUIRE(r.first[0].Key == 64 && r.first[1].Key == 68 && r.first[2].Key == 60 && r.first[3].Key == 72, "keys");
    // every live row: the plain exact search
    auto all = g.SearchFilteredExact({64.4f}, 4, nullptr);
    auto exact = g.Search({64.4f}, 4, MHNSW_MODE_EXACT);
    REQUIRE(!all.second && !exact.second && all.first == exact.first, "unfiltered");
    // more than the filter holds: every allowed row, once
    r = g.SearchFilteredExact({0.f}, 100, &f);
    REQUIRE(!r.second && r.first.size() == 75 && r.first[74].Key == 296, "whole filter");
    // a deleted row is never returned; an empty filter answers nothing
    REQUIRE(g.Delete(64), "delete");
    r = g.SearchFilteredExact({64.4f}, 1, &f);
    REQUIRE(!r.second && r.first.size() == 1 && r.first[0].Key == 68, "after delete");
    auto none = g.MakeFilter({});
    r = g.SearchFilteredExact({64.4f}, 3, &none);
    REQUIRE(!r.second && r.first.empty(), "empty filter");
    // errors
    auto e = g.SearchFilteredExact({64.4f}, 257, &f);
    REQUIRE(e.second.code == MHNSW_EUNSUPPORTED && e.second.msg == "exact mode supports k <= 256", "k");
    e = g.SearchFilteredExact({1.f, 2.f}, 4, &f);
    REQUIRE(e.second.code == MHNSW_EDIM, "dim");
    f.Close();
    e = g.SearchFilteredExact({64.4f}, 4, &f);
    REQUIRE(e.second.code == MHNSW_EINVAL, "closed filter");
}

int main() {
    TestSearchFilteredExact();
    if (failures == 0) std::printf("PASS\n");
    return failures;
}
