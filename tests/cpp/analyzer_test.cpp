// The C++ shim's Analyzer (include/hnsw_amd/graph.hpp hnsw::Analyzer<K>, Graph<K>::Relink) over
// the C ABI: analyzer_test.go's TestAnalyzer_QualityMetrics and TestAnalyzer_EmptyGraph
// re-expressed, plus Hops, Reachability and Relink.  Compiled by tests/test_cpp_analyzer.py and
// run there on the GPU.  Exit code = failures.
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

// graph_test.go:76-84 newTestGraph
static void TestAnalyzer_QualityMetrics() {
    hnsw::Graph<int> g(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    hnsw::Analyzer<int> analyzer{&g};
    auto m = analyzer.QualityMetrics();
    REQUIRE(!m.second && m.first.NodeCount == 0, "empty NodeCount");
    REQUIRE(m.first.AvgConnectivity == 0.0 && m.first.ConnectivityStdDev == 0.0, "empty connectivity");
    for (int i = 0; i < 100; ++i) REQUIRE(!g.Add(hnsw::MakeNode(i, {(float)i})), "add");
    m = analyzer.QualityMetrics();
    REQUIRE(!m.second, "metrics");
    REQUIRE(m.first.NodeCount == 100, "NodeCount");
    REQUIRE(m.first.AvgConnectivity > 0.0 && m.first.AvgConnectivity <= 6.0, "AvgConnectivity");
    REQUIRE(m.first.ConnectivityStdDev >= 0.0, "ConnectivityStdDev");
    REQUIRE(m.first.GraphHeight >= 1 && m.first.GraphHeight == analyzer.Height(), "GraphHeight");
    REQUIRE(m.first.LayerBalance >= 0.0 && m.first.LayerBalance <= 1.0, "LayerBalance");
    REQUIRE(m.first.DistortionRatio >= 0.0, "DistortionRatio");
    REQUIRE(m.first.AvgConnectivity == analyzer.Connectivity()[0], "Connectivity delegate");
    REQUIRE(analyzer.Topography() == g.Topography() && analyzer.Topography()[0] == 100, "Topography delegate");
    auto h = analyzer.DegreeHistogram(0);
    int64_t rows = 0, edges = 0;
    for (size_t d = 0; d < h.first.size(); ++d) rows += h.first[d], edges += h.first[d] * (int64_t)d;
    REQUIRE(!h.second && rows == 100 && (double)edges / 100.0 == m.first.AvgConnectivity, "DegreeHistogram");
    // analyzer_test.go:50-87: distance to self is 0, others are not negative here
    auto hp = analyzer.Hops({0, 1, 3});
    REQUIRE(!hp.second && hp.first.size() == 9, "Hops");
    REQUIRE(hp.first[0] == 0 && hp.first[4] == 0 && hp.first[8] == 0, "Hops diagonal");
    REQUIRE(hp.first[1] >= -1 && hp.first[1] <= 10, "Hops range");
    auto bad = analyzer.Hops({0, 1, 1});
    REQUIRE(bad.second.code == MHNSW_EINVAL, "Hops repeated key");
    auto r = analyzer.Reachability();
    REQUIRE(!r.second && (int)r.first.members.size() == analyzer.Height() && r.first.members[0] == 100, "Reachability");
    REQUIRE((int64_t)r.first.unreachable_keys.size() == r.first.members[0] - r.first.reached[0], "unreachable count");
    // a compat handle refuses Relink with update's message
    auto rl = g.Relink({1, 2});
    REQUIRE(rl.second.code == MHNSW_EUNSUPPORTED &&
                rl.second.msg == "update needs a batch or flat (build_mode 1 or 2) handle",
            "compat Relink refusal");
}

static void TestAnalyzer_EmptyGraph() {
    hnsw::Graph<int> g(6, 0.5, 20, &hnsw::EuclideanDistance, 0);
    hnsw::Analyzer<int> analyzer{&g};
    auto m = analyzer.QualityMetrics();
    REQUIRE(!m.second, "metrics");
    REQUIRE(m.first.NodeCount == 0 && m.first.GraphHeight == 0, "counts");
    REQUIRE(m.first.AvgConnectivity == 0.0 && m.first.ConnectivityStdDev == 0.0 && m.first.DistortionRatio == 0.0 &&
                m.first.LayerBalance == 0.0,
            "metrics all zero");
    REQUIRE(analyzer.Height() == 0 && analyzer.Topography().empty() && analyzer.Connectivity().empty(), "delegates");
    auto r = analyzer.Reachability();
    REQUIRE(!r.second && r.first.members.empty() && r.first.unreachable_keys.empty(), "Reachability");
    auto rp = analyzer.Repair();
    REQUIRE(!rp.second && rp.first.first == 0 && rp.first.second == 0, "Repair");
}

// a batch-mode graph: Relink keeps the vectors and reports the found keys; Repair reports counts
static void TestRelink() {
    hnsw::Graph<std::string> g(8, 0.4, 32, &hnsw::EuclideanDistance, 0);
    REQUIRE(!g.SetOption("build_mode", MHNSW_BUILD_BATCH), "batch mode");
    std::vector<hnsw::Node<std::string>> nodes;
    char name[16];
    for (int i = 0; i < 300; ++i) {
        std::snprintf(name, sizeof name, "k%03d", i);
        nodes.push_back(hnsw::MakeNode(std::string(name), {(float)i, 0.5f}));
    }
    REQUIRE(!g.BatchAdd(nodes), "add");
    const std::vector<float> q = {100.2f, 0.f};
    auto s0 = g.Search(q, 10, MHNSW_MODE_EXACT);
    auto rl = g.Relink({"k005", "zzz", "k299"});
    REQUIRE(!rl.second && rl.first.size() == 3 && rl.first[0] && !rl.first[1] && rl.first[2], "Relink found");
    int64_t rows = -1;
    REQUIRE(mhnsw_get_option(g.handle(), "last_update_rows", &rows) == 0 && rows == 2, "last_update_rows");
    auto s1 = g.Search(q, 10, MHNSW_MODE_EXACT);
    REQUIRE(!s0.second && !s1.second && s0.first == s1.first, "vectors unchanged");
    auto dup = g.Relink({"k005", "k005"});
    REQUIRE(dup.second.code == MHNSW_EINVAL, "repeated key");
    hnsw::Analyzer<std::string> analyzer{&g};
    auto before = analyzer.Reachability();
    auto rp = analyzer.Repair();
    REQUIRE(!before.second && !rp.second && rp.first.first == (int64_t)before.first.unreachable_keys.size(), "Repair before");
    auto after = analyzer.Reachability();
    REQUIRE(!after.second && rp.first.second == (int64_t)after.first.unreachable_keys.size(), "Repair after");
    auto hp = analyzer.Hops({"k000", "k001"});
    REQUIRE(!hp.second && hp.first.size() == 4 && hp.first[0] == 0 && hp.first[3] == 0, "Hops string keys");
}

int main() {
    TestAnalyzer_QualityMetrics();
    TestAnalyzer_EmptyGraph();
    TestRelink();
    if (failures == 0) std::printf("PASS\n");
    return failures;
}
