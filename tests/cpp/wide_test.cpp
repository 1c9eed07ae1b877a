// The C++ shim's exact search past k 256 (include/hnsw_amd/graph.hpp Graph<K>::Search /
// SearchFilteredExact with the option "exact_wide") over the C ABI.  Compiled by
// tests/test_cpp_wide.py and run there on the GPU.  Exit code = failures.
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

// 1000 points on a line, query at 0: the k nearest are the keys 0 .. k - 1 in order
static void TestWideSearch() {
    hnsw::Graph<int> g(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    std::vector<hnsw::Node<int>> nodes;
    for (int i = 0; i < 1000; ++i) nodes.push_back(hnsw::MakeNode(i, {(float)i}));
    REQUIRE(!g.BatchAdd(nodes), "add");
    auto e = g.Search({0.0f}, 300, MHNSW_MODE_EXACT);
    REQUIRE(e.second.code == MHNSW_EUNSUPPORTED && e.second.msg == "exact mode supports k <= 256", "off by default");
    REQUIRE(!g.SetOption("exact_wide", 1), "set_option");
    for (int k : {257, 300, 1000, 4096}) {
        auto r = g.Search({0.0f}, k, MHNSW_MODE_EXACT);
        const size_t want = k < 1000 ? (size_t)k : 1000;
        REQUIRE(!r.second && r.first.size() == want, "len");
        bool ordered = r.first.size() == want;
        for (size_t i = 0; ordered && i < want; ++i) ordered = r.first[i].Key == (int)i;
        REQUIRE(ordered, "keys in distance order");
    }
    e = g.Search({0.0f}, 4097, MHNSW_MODE_EXACT);
    REQUIRE(e.second.code == MHNSW_EUNSUPPORTED && e.second.msg == "exact mode supports k <= 4096", "past 4096");
    // filtered: the even keys
    std::vector<int> even;
    for (int i = 0; i < 1000; i += 2) even.push_back(i);
    auto f = g.MakeFilter(even);
    auto r = g.SearchFilteredExact({0.0f}, 400, &f);
    REQUIRE(!r.second && r.first.size() == 400, "filtered len");
    bool ok = r.first.size() == 400;
    for (size_t i = 0; ok && i < 400; ++i) ok = r.first[i].Key == (int)(2 * i);
    REQUIRE(ok, "filtered keys");
    r = g.SearchFilteredExact({0.0f}, 600, &f);
    REQUIRE(!r.second && r.first.size() == 500, "filtered: fewer allowed rows than k");
    // a deleted row is never returned
    REQUIRE(g.Delete(3), "delete");
    r = g.Search({0.0f}, 300, MHNSW_MODE_EXACT);
    REQUIRE(!r.second && r.first.size() == 300 && r.first[3].Key == 4 && r.first[299].Key == 300, "after delete");
    // string keys
    hnsw::Graph<std::string> s(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    std::vector<hnsw::Node<std::string>> sn;
    for (int i = 0; i < 400; ++i) sn.push_back(hnsw::MakeNode(std::string("k") + std::to_string(1000 + i), {(float)i}));
    REQUIRE(!s.BatchAdd(sn), "add strings");
    REQUIRE(!s.SetOption("exact_wide", 1), "set_option");
    auto sr = s.Search({0.0f}, 260, MHNSW_MODE_EXACT);
    REQUIRE(!sr.second && sr.first.size() == 260 && sr.first[0].Key == "k1000" && sr.first[259].Key == "k1259", "string keys");
}

int main() {
    TestWideSearch();
    if (failures == 0) std::printf("PASS\n");
    return failures;
}
