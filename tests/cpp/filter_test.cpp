// The C++ shim's filtered search (include/hnsw_amd/graph.hpp Graph<K>::Filter,
// SearchFiltered) over the C ABI.  Compiled and run by tests/test_cpp_filter.py
// (GPU).  Exit code = failures.
#include <cstdio>
#include <set>
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

// 128 points on a line; the filter allows the multiples of 4
static void TestSearchFiltered() {
    hnsw::Graph<int> g(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    for (int i = 0; i < 128; ++i) REQUIRE(!g.Add(hnsw::MakeNode(i, {(float)i})), "add");
    std::vector<int> fours;
    for (int i = 0; i < 128; i += 4) fours.push_back(i);
    fours.push_back(1000);  // an absent key is ignored
    {
        auto f = g.MakeFilter(fours);
        REQUIRE(!f.Err() && f.Id() >= 0, "create");
        auto c = f.Count();
        REQUIRE(!c.second && c.first == 32, "count");
        auto r = g.SearchFiltered({64.4f}, 4, &f, 20, 128);
        REQUIRE(!r.second && r.first.size() == 4, "len");
        if (r.first.size() == 4) {
            REQUIRE(r.first[0].Key == 64 && r.first[1].Key == 68 && r.first[2].Key == 60 && r.first[3].Key == 72, "keys");
            REQUIRE(r.first[0].Value == hnsw::Vector{64.f}, "value");
        }
        // every live row: the plain beam search
        auto all = g.SearchFiltered({64.4f}, 4, nullptr, 20, 128);
        auto beam = g.Search({64.4f}, 4, MHNSW_MODE_BEAM);
        REQUIRE(!all.second && !beam.second && all.first == beam.first, "unfiltered");
        // update
        REQUIRE(!f.Remove({64}), "remove");
        REQUIRE(f.Count().first == 31, "count after remove");
        r = g.SearchFiltered({64.4f}, 1, &f, 20, 128);
        REQUIRE(!r.second && r.first.size() == 1 && r.first[0].Key == 68, "after remove");
        REQUIRE(!f.Add({65}), "add key");
        r = g.SearchFiltered({64.4f}, 1, &f, 20, 128);
        REQUIRE(!r.second && r.first.size() == 1 && r.first[0].Key == 65, "after add");
        // a deleted row is never returned, though its bit stays
        REQUIRE(g.Delete(65), "delete");
        r = g.SearchFiltered({64.4f}, 1, &f, 20, 128);
        REQUIRE(!r.second && r.first.size() == 1 && r.first[0].Key == 68, "after delete");
        // errors
        auto e = g.SearchFiltered({64.4f}, 4, &f, 129, 0);
        REQUIRE(e.second.code == MHNSW_EUNSUPPORTED && e.second.msg == "filtered search supports max(ef,k) <= 128", "ef");
        e = g.SearchFiltered({64.4f}, 4, &f, 20, 2049);
        REQUIRE(e.second.code == MHNSW_EUNSUPPORTED && e.second.msg == "filtered search supports route <= 2048", "route");
        e = g.SearchFiltered({1.f, 2.f}, 4, &f);
        REQUIRE(e.second.code == MHNSW_EDIM, "dim");
        const int id = f.Id();
        f.Close();
        REQUIRE(f.Id() < 0, "closed");
        e = g.SearchFiltered({64.4f}, 4, &f);
        REQUIRE(e.second.code == MHNSW_EINVAL, "closed filter");
        int64_t n = 0;
        REQUIRE(mhnsw_filter_count(g.handle(), id, &n) == MHNSW_EINVAL, "destroyed id");
        REQUIRE(std::string(mhnsw_last_error(g.handle())) == "unknown filter " + std::to_string(id), "destroyed id text");
    }
    // a filter of another graph is refused, not read against this graph's handle
    {
        hnsw::Graph<int> other(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
        REQUIRE(!other.Add(hnsw::MakeNode(1, {1.f})), "other add");
        auto fo = other.MakeFilter({1});
        auto e = g.SearchFiltered({64.4f}, 4, &fo);
        REQUIRE(e.second.code == MHNSW_EINVAL && e.second.msg == "filter of another graph", "other graph's filter");
        auto ok = other.SearchFiltered({1.f}, 1, &fo);
        REQUIRE(!ok.second && ok.first.size() == 1 && ok.first[0].Key == 1, "own filter");
    }
    // the destructor releases the slot: the next filter takes it again
    int first;
    {
        auto a = g.MakeFilter({1, 2, 3});
        first = a.Id();
    }
    auto b = g.MakeFilter({4});
    REQUIRE(b.Id() == first, "slot reuse");
}

static void TestStringKeys() {
    hnsw::Graph<std::string> g(8, 0.25, 20, &hnsw::CosineDistance, 3);
    const char* names[] = {"apple", "banana", "cherry", "date", "elder", "fig"};
    for (int i = 0; i < 6; ++i)
        REQUIRE(!g.Add(hnsw::MakeNode(std::string(names[i]), {1.f, (float)i, 0.5f})), "add");
    auto f = g.MakeFilter({"banana", "date", "fig", "grape"});
    REQUIRE(!f.Err() && f.Count().first == 3, "count");
    auto r = g.SearchFiltered({1.f, 0.f, 0.5f}, 6, &f, 20, 64);
    REQUIRE(!r.second && r.first.size() == 3, "len");
    std::set<std::string> got;
    for (const auto& n : r.first) got.insert(n.Key);
    REQUIRE(got == (std::set<std::string>{"banana", "date", "fig"}), "keys");
    if (!r.first.empty()) REQUIRE(r.first[0].Key == "banana", "nearest");
}

int main() {
    TestSearchFiltered();
    TestStringKeys();
    if (failures == 0) std::printf("PASS\n");
    return failures;
}
