// The C++ shim's LSH index (include/hnsw_amd/graph.hpp Graph<K>::EnableLSH / SearchLSH) over the
// C ABI.  Compiled by tests/test_cpp_lsh.py and run there on the GPU.  Exit code = failures.
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

// 200 points (i - 99.5, 1): the projections (1, 0) and (0, 1), one table of one bit each, put a
// point in the query's bucket of table 0 iff it lies on the query's side of x = 0, and every
// point in the query's bucket of table 1
static void TestLSH() {
    hnsw::Graph<int> g(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    auto e = g.SearchLSH({1.f, 1.f}, 3);
    REQUIRE(e.second.code == MHNSW_EINVAL && e.second.msg == "LSH search before mhnsw_lsh_enable", "before enable");
    for (int i = 0; i < 200; ++i) REQUIRE(!g.Add(hnsw::MakeNode(i, {(float)i - 99.5f, 1.f})), "add");
    REQUIRE(g.EnableLSH(33, 1).code == MHNSW_EINVAL && g.EnableLSH(1, 1, 42, {1.f, 0.f, 0.f}, 2).code == MHNSW_EINVAL,
            "refusals");
    REQUIRE(!g.EnableLSH(1, 1, 42, {1.f, 0.f}, 2), "enable on a handle that holds rows");
    auto r = g.SearchLSH({-3.2f, 1.f}, 4);  // nearest overall: 96 (-3.5), 97 (-2.5), 95, 98
    REQUIRE(!r.second && r.first.Candidates == 100 && r.first.Nodes.size() == 4, "left half");
    if (r.first.Nodes.size() == 4)
        REQUIRE(r.first.Nodes[0].Key == 96 && r.first.Nodes[1].Key == 97 && r.first.Nodes[2].Key == 95 &&
                    r.first.Nodes[3].Key == 98 && r.first.Distances[0] > 0.29f && r.first.Distances[0] < 0.31f,
                "keys by distance");
    r = g.SearchLSH({0.2f, 1.f}, 3);  // 99 (-0.5) is nearer than 101 (1.5) but across the hyperplane
    REQUIRE(!r.second && r.first.Nodes.size() == 3 && r.first.Nodes[0].Key == 100 && r.first.Nodes[1].Key == 101 &&
                r.first.Nodes[2].Key == 102,
            "the bucket only");
    REQUIRE(g.Delete(100), "delete");
    r = g.SearchLSH({0.2f, 1.f}, 3);
    REQUIRE(!r.second && r.first.Candidates == 99 && r.first.Nodes.size() == 3 && r.first.Nodes[0].Key == 101, "deleted");
    REQUIRE(!g.EnableLSH(2, 1, 42, {1.f, 0.f, 0.f, 1.f}, 2), "enable again, another shape");
    r = g.SearchLSH({0.2f, 1.f}, 3);  // table 1 (y > 0) holds every row, each counted once
    REQUIRE(!r.second && r.first.Candidates == 199 && r.first.Nodes.size() == 3 && r.first.Nodes[0].Key == 99, "two tables");
    e = g.SearchLSH({0.2f, 1.f}, 257);
    REQUIRE(e.second.code == MHNSW_EUNSUPPORTED && e.second.msg == "LSH search supports k <= 256", "k limit");
    e = g.SearchLSH({0.2f}, 3);
    REQUIRE(e.second.code == MHNSW_EDIM, "dim");
    // string keys, generated projections
    hnsw::Graph<std::string> s(6, 0.5, 20, &hnsw::CosineDistance, 0);
    REQUIRE(!s.EnableLSH(4, 2), "enable before the first add");
    for (int i = 0; i < 40; ++i)
        REQUIRE(!s.Add(hnsw::MakeNode(std::string("k") + std::to_string(100 + i), {(float)(i % 7) - 3.f, (float)i, 1.f})), "add");
    auto sr = s.SearchLSH({-3.f, 0.f, 1.f}, 1);  // its own row shares every bucket with it
    REQUIRE(!sr.second && sr.first.Nodes.size() == 1 && sr.first.Nodes[0].Key == "k100" && sr.first.Candidates >= 1,
            "string keys");
}

int main() {
    TestLSH();
    if (failures == 0) std::printf("PASS\n");
    return failures;
}
