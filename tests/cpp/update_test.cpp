// The C++ shim's in-place update (include/hnsw_amd/graph.hpp Graph<K>::Update / Upsert) over
// the C ABI.  Compiled by tests/test_cpp_update.py and run there on the GPU.  Exit code = failures.
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

// 400 points on a line in a batch-mode graph; keys 10, 200 and 399 move far away
static void TestUpdate() {
    hnsw::Graph<int> g(8, 0.4, 32, &hnsw::EuclideanDistance, 0);
    REQUIRE(!g.SetOption("build_mode", MHNSW_BUILD_BATCH), "batch mode");
    std::vector<hnsw::Node<int>> nodes;
    for (int i = 0; i < 400; ++i) nodes.push_back(hnsw::MakeNode(i, {(float)i, 0.5f}));
    REQUIRE(!g.BatchAdd(nodes), "add");
    std::vector<int> evens;
    for (int i = 0; i < 400; i += 2) evens.push_back(i);
    auto f = g.MakeFilter(evens);
    REQUIRE(!f.Err(), "filter");
    REQUIRE(g.Delete(50), "delete");
    int64_t cap0 = 0, cap1 = 0, dead = -1, rows = -1, chunks = -1;
    mhnsw_get_option(g.handle(), "capacity", &cap0);
    auto u = g.Update({hnsw::MakeNode(10, {1010.f, 0.5f}), hnsw::MakeNode(200, {1200.f, 0.5f}),
                       hnsw::MakeNode(50, {1050.f, 0.5f}), hnsw::MakeNode(7777, {1.f, 0.5f}),
                       hnsw::MakeNode(399, {1399.f, 0.5f})});
    REQUIRE(!u.second, "update");
    REQUIRE(u.first == std::vector<bool>({true, true, false, false, true}), "found flags");
    REQUIRE(g.Len() == 399, "Len");
    mhnsw_get_option(g.handle(), "capacity", &cap1);
    REQUIRE(cap0 == cap1, "capacity");
    REQUIRE(mhnsw_get_option(g.handle(), "dead_rows", &dead) == 0 && dead == 1, "dead_rows");
    REQUIRE(mhnsw_get_option(g.handle(), "last_update_rows", &rows) == 0 && rows == 3, "last_update_rows");
    REQUIRE(mhnsw_get_option(g.handle(), "last_update_chunks", &chunks) == 0 && chunks >= 1, "last_update_chunks");
    for (int k : {10, 200, 399}) {
        auto s = g.Search({1000.f + (float)k + 0.1f, 0.5f}, 1, MHNSW_MODE_BEAM);
        REQUIRE(!s.second && s.first.size() == 1 && s.first[0].Key == k, "the new vector's key first");
        auto v = g.Lookup(k);
        REQUIRE(v.second && v.first == hnsw::Vector({1000.f + (float)k, 0.5f}), "Lookup");
    }
    auto s0 = g.Search({10.1f, 0.5f}, 1, MHNSW_MODE_BEAM);
    REQUIRE(!s0.second && s0.first.size() == 1 && s0.first[0].Key != 10, "the old vector is gone");
    // the row kept its filter bit: key 10 and 200 are even
    auto x = g.SearchFilteredExact({1200.2f, 0.5f}, 1, &f);
    REQUIRE(!x.second && x.first.size() == 1 && x.first[0].Key == 200, "filter bit kept");
    // Upsert: 10 present, 50 (deleted) and 7777 absent
    auto w = g.Upsert({hnsw::MakeNode(10, {2010.f, 0.5f}), hnsw::MakeNode(50, {2050.f, 0.5f}),
                       hnsw::MakeNode(7777, {2077.f, 0.5f})});
    REQUIRE(!w.second && w.first == std::vector<bool>({true, false, false}), "upsert flags");
    REQUIRE(g.Len() == 401, "Len after upsert");
    for (int k : {10, 50}) {
        auto s = g.Search({2000.f + (float)k + 0.1f, 0.5f}, 1, MHNSW_MODE_BEAM);
        REQUIRE(!s.second && s.first.size() == 1 && s.first[0].Key == k, "upserted key first");
    }
    // a repeated key, a compat handle
    auto r = g.Update({hnsw::MakeNode(3, {1.f, 0.5f}), hnsw::MakeNode(3, {2.f, 0.5f})});
    REQUIRE(r.second.code == MHNSW_EINVAL && r.second.msg == "duplicate key 3 in update", "repeated key");
    hnsw::Graph<int> cg(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    REQUIRE(!cg.Add(hnsw::MakeNode(1, {1.f})), "compat add");
    auto e = cg.Update({hnsw::MakeNode(1, {2.f})});
    REQUIRE(e.second.code == MHNSW_EUNSUPPORTED &&
                e.second.msg == "update needs a batch or flat (build_mode 1 or 2) handle",
            "compat refusal");
}

// string keys go through the order labels: an unknown string is absent
static void TestStringKeys() {
    hnsw::Graph<std::string> g(8, 0.4, 32, &hnsw::EuclideanDistance, 0);
    REQUIRE(!g.SetOption("build_mode", MHNSW_BUILD_BATCH), "batch mode");
    std::vector<hnsw::Node<std::string>> nodes;
    for (int i = 0; i < 60; ++i) nodes.push_back(hnsw::MakeNode(std::string("k") + std::to_string(i), {(float)i, 1.f}));
    REQUIRE(!g.BatchAdd(nodes), "add");
    auto u = g.Upsert({hnsw::MakeNode(std::string("k7"), {507.f, 1.f}), hnsw::MakeNode(std::string("new-a"), {600.f, 1.f}),
                       hnsw::MakeNode(std::string("new-b"), {700.f, 1.f})});
    REQUIRE(!u.second && u.first == std::vector<bool>({true, false, false}), "string upsert");
    REQUIRE(g.Len() == 62, "Len");
    auto s = g.Search({507.2f, 1.f}, 1, MHNSW_MODE_BEAM);
    REQUIRE(!s.second && s.first.size() == 1 && s.first[0].Key == "k7", "string key first");
}

int main() {
    TestUpdate();
    TestStringKeys();
    if (failures == 0) std::printf("PASS\n");
    return failures;
}
