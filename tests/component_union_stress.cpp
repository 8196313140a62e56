// component_union_stress — the union–find of gs4d_label_components (csrc/component_union.h, the text the kernels compile) under real contention on
// the CPU: 16 std::threads unite the shuffled edges of known graphs through std::atomic with relaxed ordering, as the kernel's lanes do through
// agent-scope atomics, then every node's root is checked against the smallest node of its component, computed by a sequential flood fill.
// A program of its own (tests/test_components_host.py builds it with -fsanitize=thread where that runtime exists and runs it); prints one line per
// graph and exits 0 iff every label is right and no trip bound ran out.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <thread>
#include <utility>
#include <vector>

#include "../4dgaussiansplatrendering_amd/csrc/component_union.h"

namespace {

constexpr int THREADS = 16;
using Edge = std::pair<uint32_t, uint32_t>;

struct AtomicParents {
    std::atomic<uint32_t>* p;
    uint32_t load(uint32_t x) const { return p[x].load(std::memory_order_relaxed); }
    bool cas(uint32_t x, uint32_t is, uint32_t to) { return p[x].compare_exchange_strong(is, to, std::memory_order_relaxed); }
    void lower(uint32_t x, uint32_t v) {
        uint32_t cur = p[x].load(std::memory_order_relaxed);
        while (v < cur && !p[x].compare_exchange_weak(cur, v, std::memory_order_relaxed)) {}
    }
};

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rng() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }

// the smallest node of every node's component, by a sequential flood fill over adjacency lists
std::vector<uint32_t> expected(uint32_t n, const std::vector<Edge>& edges) {
    std::vector<std::vector<uint32_t>> adj(n);
    for (const Edge& e : edges) { adj[e.first].push_back(e.second); adj[e.second].push_back(e.first); }
    std::vector<uint32_t> label(n, 0xFFFFFFFFu), stack;
    for (uint32_t s = 0; s < n; ++s) {
        if (label[s] != 0xFFFFFFFFu) continue;
        label[s] = s; stack.push_back(s);                        // (s ascends: the first node of a component to be met is its smallest)
        while (!stack.empty()) {
            const uint32_t x = stack.back(); stack.pop_back();
            for (uint32_t y : adj[x]) if (label[y] == 0xFFFFFFFFu) { label[y] = s; stack.push_back(y); }
        }
    }
    return label;
}

bool run(const char* name, uint32_t n, std::vector<Edge> edges) {
    for (size_t k = edges.size(); k > 1; --k) std::swap(edges[k - 1], edges[rng() % k]);
    std::unique_ptr<std::atomic<uint32_t>[]> parent(new std::atomic<uint32_t>[n]);
    for (uint32_t x = 0; x < n; ++x) parent[x].store(x, std::memory_order_relaxed);
    std::atomic<int> overruns{ 0 };
    std::vector<std::thread> pool;
    for (int t = 0; t < THREADS; ++t)
        pool.emplace_back([&, t] {
            AtomicParents mem{ parent.get() };
            for (size_t k = (size_t)t; k < edges.size(); k += THREADS)          // interleaved: neighbouring edges go to different threads
                if (!gs4d_union::unite(mem, edges[k].first, edges[k].second, n)) overruns.fetch_add(1, std::memory_order_relaxed);
        });
    for (std::thread& th : pool) th.join();
    // the flatten step, concurrent too
    std::vector<uint32_t> got(n);
    pool.clear();
    for (int t = 0; t < THREADS; ++t)
        pool.emplace_back([&, t] {
            AtomicParents mem{ parent.get() };
            for (uint32_t x = (uint32_t)t; x < n; x += THREADS) {
                const uint32_t root = gs4d_union::find(mem, x, n);
                if (root == gs4d_union::OVERRUN) { overruns.fetch_add(1, std::memory_order_relaxed); continue; }
                mem.lower(x, root);
                got[x] = root;
            }
        });
    for (std::thread& th : pool) th.join();
    const std::vector<uint32_t> want = expected(n, edges);
    size_t wrong = 0, components = 0;
    for (uint32_t x = 0; x < n; ++x) {
        wrong += got[x] != want[x] || parent[x].load(std::memory_order_relaxed) != want[x];
        components += want[x] == x;
    }
    std::printf("%-10s n = %u, %zu edges, %zu components: %zu wrong, %d overruns\n", name, n, edges.size(), components, wrong, overruns.load());
    return wrong == 0 && overruns.load() == 0;
}

} // namespace

int main() {
    bool ok = true;
    {   // a chain: the longest find paths
        const uint32_t n = 20000;
        std::vector<Edge> e;
        for (uint32_t x = 1; x < n; ++x) e.push_back({ x, x - 1 });
        ok &= run("chain", n, e);
    }
    {   // a clump: every pair, all hooking onto one root
        const uint32_t n = 256;
        std::vector<Edge> e;
        for (uint32_t x = 0; x < n; ++x) for (uint32_t y = 0; y < x; ++y) e.push_back({ x, y });
        ok &= run("clump", n, e);
    }
    {   // clumps of sizes 1 .. 64 with interleaved indices, and nodes nobody names
        std::vector<std::vector<uint32_t>> groups(64);
        uint32_t n = 0;
        for (uint32_t round = 0; round < 64; ++round) for (uint32_t g = round; g < 64; ++g) groups[g].push_back(n++);
        n += 100;
        std::vector<Edge> e;
        for (const auto& g : groups) for (size_t a = 0; a < g.size(); ++a) for (size_t b = 0; b < a; ++b) e.push_back({ g[a], g[b] });
        ok &= run("clumps", n, e);
    }
    {   // a grid of 200 x 200 cut into slabs, its nodes renamed by a random permutation
        const uint32_t side = 200, n = side * side;
        std::vector<uint32_t> name(n);
        for (uint32_t x = 0; x < n; ++x) name[x] = x;
        for (uint32_t k = n; k > 1; --k) std::swap(name[k - 1], name[rng() % k]);
        std::vector<Edge> e;
        for (uint32_t y = 0; y < side; ++y) for (uint32_t x = 0; x < side; ++x) {
            if (x + 1 < side) e.push_back({ name[y * side + x], name[y * side + x + 1] });
            if (y + 1 < side && y % 37 != 36) e.push_back({ name[y * side + x], name[(y + 1) * side + x] });
        }
        ok &= run("slabs", n, e);
    }
    {   // a sparse random graph: many components of every size
        const uint32_t n = 50000;
        std::vector<Edge> e;
        for (uint32_t k = 0; k < n / 2 + n / 8; ++k) { const uint32_t a = rng() % n, b = rng() % n; if (a != b) e.push_back({ a, b }); }
        ok &= run("random", n, e);
    }
    std::printf(ok ? "component_union_stress: ok\n" : "component_union_stress: FAILED\n");
    return ok ? 0 : 1;
}
