// The C++ shim's compaction (include/hnsw_amd/graph.hpp Graph<K>::Compact) over the C ABI.
// Compiled by tests/test_cpp_compact.py and run there on the GPU.  Exit code = failures.
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

template <class N>
static bool same_nodes(const std::vector<N>& a, const std::vector<N>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].Key != b[i].Key || a[i].Value != b[i].Value) return false;
    return true;
}

// 400 points on a line in a batch-mode graph; every third key of 30..329 deleted
static void TestCompact() {
    hnsw::Graph<int> g(8, 0.4, 32, &hnsw::EuclideanDistance, 0);
    REQUIRE(!g.SetOption("build_mode", MHNSW_BUILD_BATCH), "batch mode");
    std::vector<hnsw::Node<int>> nodes;
    for (int i = 0; i < 400; ++i) nodes.push_back(hnsw::MakeNode(i, {(float)i, 0.5f}));
    REQUIRE(!g.BatchAdd(nodes), "add");
    std::vector<int> evens, gone;
    for (int i = 0; i < 400; i += 2) evens.push_back(i);
    for (int i = 30; i < 330; i += 3) gone.push_back(i);
    auto f = g.MakeFilter(evens);
    REQUIRE(!f.Err(), "filter");
    for (bool ok : g.BatchDelete(gone)) REQUIRE(ok, "delete");
    const std::vector<float> q = {100.2f, 0.f};
    auto s0 = g.Search(q, 10, MHNSW_MODE_BEAM);
    auto f0 = g.SearchFiltered(q, 10, &f);
    auto x0 = g.SearchFilteredExact(q, 10, &f);
    auto r0 = g.RangeSearch(q, 6.0f);
    REQUIRE(!s0.second && !f0.second && !x0.second && !r0.second, "searches before");
    int64_t dead = -1, cap0 = 0, cap1 = 0;
    REQUIRE(mhnsw_get_option(g.handle(), "dead_rows", &dead) == 0 && dead == 100, "dead_rows before");
    mhnsw_get_option(g.handle(), "capacity", &cap0);
    auto c = g.Compact();
    REQUIRE(!c.second && c.first == 100, "rows removed");
    REQUIRE(g.Len() == 300, "Len");
    REQUIRE(mhnsw_get_option(g.handle(), "dead_rows", &dead) == 0 && dead == 0, "dead_rows after");
    mhnsw_get_option(g.handle(), "capacity", &cap1);
    REQUIRE(cap0 == cap1, "capacity");
    auto s1 = g.Search(q, 10, MHNSW_MODE_BEAM);
    auto f1 = g.SearchFiltered(q, 10, &f);
    auto x1 = g.SearchFilteredExact(q, 10, &f);
    auto r1 = g.RangeSearch(q, 6.0f);
    REQUIRE(!s1.second && same_nodes(s0.first, s1.first) && s1.first.size() == 10, "Search unchanged");
    REQUIRE(!f1.second && same_nodes(f0.first, f1.first) && f1.first.size() == 10, "SearchFiltered unchanged");
    REQUIRE(!x1.second && same_nodes(x0.first, x1.first), "SearchFilteredExact unchanged");
    REQUIRE(!r1.second && r0.first.size() == r1.first.size() && !r1.first.empty(), "RangeSearch count");
    for (size_t i = 0; i < r1.first.size() && i < r0.first.size(); ++i)
        REQUIRE(r0.first[i].node.Key == r1.first[i].node.Key && r0.first[i].Distance == r1.first[i].Distance,
                "RangeSearch unchanged");
    // nothing left to remove; a deleted key comes back into a freed row
    c = g.Compact();
    REQUIRE(!c.second && c.first == 0, "second call");
    REQUIRE(!g.Add(hnsw::MakeNode(30, {30.f, 0.5f})), "re-add");
    auto s2 = g.Search({30.1f, 0.5f}, 1, MHNSW_MODE_BEAM);
    REQUIRE(!s2.second && s2.first.size() == 1 && s2.first[0].Key == 30, "re-added key found");
    auto f2 = g.SearchFilteredExact({30.1f, 0.5f}, 1, &f);
    REQUIRE(!f2.second && f2.first.size() == 1 && f2.first[0].Key != 30, "a freed row's filter bit is clear");
    // a compat handle refuses
    hnsw::Graph<int> cg(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    REQUIRE(!cg.Add(hnsw::MakeNode(1, {1.f})), "compat add");
    auto e = cg.Compact();
    REQUIRE(e.second.code == MHNSW_EUNSUPPORTED &&
                e.second.msg == "compact needs a batch or flat (build_mode 1 or 2) handle",
            "compat refusal");
}

int main() {
    TestCompact();
    if (failures == 0) std::printf("PASS\n");
    return failures;
}
