// test_ragged_rebuild.cc -- the ragged rebuild path: a staged chunk of the
// multi-fetch or the repair with several shard sizes rebuilt by ONE
// memo_ec_rebuild_ragged call per erasure count and one per shared pattern,
// every survivor staged at its own shard size ("ragged-rebuild"), and
// Codec::rebuild_ragged.  The CPU tests cover the grouping, the offset
// arithmetic of the staging and the device partition; the GPU ones run
// RS(10,4) on 16 in-process nodes.  (The small harness is restated from
// test_ragged.cc.)
//   usage: test_ragged_rebuild [--cpu-only] [filter]
#include <cstdio>
#include <cstring>
#include <random>
#include <set>

#include "../erasure_consensus.hh"

using namespace memo_host;

namespace {

struct TestCase {
  const char* name;
  bool gpu;
  void (*fn)();
};
std::vector<TestCase>& tests() {
  static std::vector<TestCase> t;
  return t;
}
struct Reg {
  Reg(const char* n, bool g, void (*f)()) { tests().push_back({n, g, f}); }
};
int g_fail = 0;

#define TEST(name, gpu)                      \
  static void test_##name();                 \
  static Reg reg_##name(#name, gpu, test_##name); \
  static void test_##name()
#define CHECK(x)                                                             \
  do {                                                                       \
    if (!(x)) {                                                              \
      std::fprintf(stderr, "  CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #x); \
      ++g_fail;                                                              \
    }                                                                        \
  } while (0)
#define CHECK_EQ(x, y)                                                       \
  do {                                                                       \
    const long long x_ = (long long)(x), y_ = (long long)(y);                \
    if (x_ != y_) {                                                          \
      std::fprintf(stderr, "  CHECK_EQ failed %s:%d: %s = %lld, %s = %lld\n", __FILE__, __LINE__, #x, \
                   x_, #y, y_);                                              \
      ++g_fail;                                                              \
    }                                                                        \
  } while (0)

Buffer random_bytes(size_t n, uint64_t seed) {
  std::mt19937_64 r(seed);
  Buffer b(n);
  for (auto& x : b) x = (uint8_t)r();
  return b;
}

void fetch_many(Consensus& c, const std::vector<Address>& as, const ReceiveBlock& res) {
  std::vector<Consensus::AddressVersion> req;
  for (auto& a : as) req.emplace_back(a, std::nullopt);
  c.fetch(req, res);
}

struct Net {
  Overlay overlay;
  std::vector<std::shared_ptr<Node>> nodes;
  std::unique_ptr<ErasureConsensus> ec;
  ErasureOptions o;
  // uniform_min: how many blocks must share a pattern to make a shared-
  // pattern batch (a huge value: per-block patterns only)
  Net(int n, int k, int m, bool ragged, int uniform_min, size_t uniform_min_bytes = 0) {
    for (int i = 0; i < n; ++i) {
      uint8_t id[32] = {0};
      id[0] = (uint8_t)(nodes.size() + 1);
      id[1] = 0x4d;
      nodes.push_back(overlay.add_node(Address(id, 0, false), make_shard_local(std::make_unique<MemorySilo>())));
    }
    o.k = k;
    o.m = m;
    o.eviction_delay_ms = -1;
    o.ragged_rebuild = ragged;
    o.uniform_min = uniform_min;
    o.uniform_min_bytes = uniform_min_bytes;
    ec = std::make_unique<ErasureConsensus>(std::make_unique<ReplicationConsensus>(overlay, 3), overlay, o);
  }
  // data shards of `a` on nodes that are down
  int lost_data(const Address& a, int k) {
    int e = 0;
    for (int i = 0; i < k; ++i)
      for (auto& n : nodes)
        if (!n->up && n->has(shard_key(a, i))) ++e;
    return e;
  }
};

// 40 blocks of 100 B .. 300 KiB, seeded (test_ragged.cc's batch).
std::vector<Block> mixed_blocks() {
  std::mt19937_64 r(0x6D656D6F);
  std::vector<Block> bs;
  for (int i = 0; i < 40; ++i) {
    const size_t B = 100 + (size_t)(r() % ((300u << 10) - 100 + 1));
    bs.push_back(make_chb(random_bytes(B, 7000 + i)));
  }
  return bs;
}

RebuildItem item(size_t S, std::initializer_list<int> surv, std::initializer_list<int> lost) {
  RebuildItem it{S, (int)lost.size(), {}};
  size_t at = 0;
  for (int s : surv) it.pat[at++] = (uint8_t)s;
  for (int l : lost) it.pat[at++] = (uint8_t)l;
  return it;
}

// Fetch every block in one multi-address request; returns how many came
// back bit-exact.
size_t multi_fetch(Net& net, const std::vector<Block>& bs) {
  std::vector<Address> req;
  for (auto& b : bs) req.push_back(b.address);
  size_t ok = 0;
  fetch_many(*net.ec, req, [&](const Address& a, std::unique_ptr<Block> b, std::exception_ptr e) {
    CHECK(b && !e);
    if (!b) return;
    for (auto& x : bs)
      if (x.address == a && b->data == x.data) ++ok;
  });
  return ok;
}

int take_down(Net& net, int want) {
  int down = 0;
  for (auto& n : net.nodes)
    if (down < want && !n->silo->list().empty()) {
      net.overlay.set_up(n->id, false);
      ++down;
    }
  return down;
}

}  // namespace

// ------------------------------------------------------------- CPU tests
// One group per e for the per-block batches of a chunk, one per shared
// pattern, whatever size buckets the planner cut them into.
TEST(groups_one_call_per_e_and_per_pattern, false) {
  const int k = 3;
  std::vector<RebuildItem> items;
  // per-block patterns, e = 1 and e = 2, in three size buckets
  items.push_back(item(64, {0, 1, 3}, {2}));       // 0
  items.push_back(item(4096, {1, 2, 4}, {0}));     // 1
  items.push_back(item(640, {0, 3, 4}, {1, 2}));   // 2
  items.push_back(item(128, {2, 3, 4}, {0, 1}));   // 3
  items.push_back(item(70000 / 64 * 64, {0, 2, 3}, {1}));  // 4
  // one pattern shared by four blocks in two buckets
  for (size_t S : {64, 8192, 64, 8256}) items.push_back(item(S, {0, 1, 2}, {4}));  // 5..8
  const std::vector<RebuildBatch> batches = plan_rebuild_batches(items, k, 256, 2, 0);
  size_t uniform = 0;
  for (auto& b : batches) uniform += b.uniform;
  CHECK(uniform >= 2);          // the shared pattern in two buckets
  CHECK(batches.size() >= 6);   // and (bucket, e) batches of the rest
  CHECK(mixed_sizes(items, batches.data(), batches.size()));
  const std::vector<RaggedRebuildGroup> gs = group_ragged_rebuilds(items, batches.data(), batches.size(), k);
  CHECK_EQ(gs.size(), 3);
  std::set<size_t> seen;
  for (const RaggedRebuildGroup& g : gs) {
    const size_t n = g.items.size();
    CHECK_EQ(g.sizes.size(), n);
    CHECK_EQ(g.off.size(), n + 1);
    CHECK_EQ(g.sidx.size(), g.uniform ? (size_t)k : n * k);
    CHECK_EQ(g.lidx.size(), g.uniform ? (size_t)g.e : n * g.e);
    size_t T = 0;
    for (size_t b = 0; b < n; ++b) {
      const RebuildItem& it = items[g.items[b]];
      CHECK(seen.insert(g.items[b]).second);
      CHECK_EQ(it.e, g.e);
      CHECK_EQ(g.sizes[b], it.S);
      CHECK_EQ(g.off[b], T);
      T += it.S;
      const uint8_t* s = g.uniform ? g.sidx.data() : g.sidx.data() + b * k;
      const uint8_t* l = g.uniform ? g.lidx.data() : g.lidx.data() + b * g.e;
      CHECK(std::equal(it.pat, it.pat + k, s) && std::equal(it.pat + k, it.pat + k + g.e, l));
    }
    CHECK_EQ(g.off[n], T);
    if (g.uniform) CHECK_EQ(n, 4);
  }
  CHECK_EQ(seen.size(), items.size());
  // one shard size only: the chunk keeps the call it made before
  std::vector<RebuildItem> same{item(4096, {0, 1, 3}, {2}), item(4096, {1, 2, 4}, {0})};
  const std::vector<RebuildBatch> sb = plan_rebuild_batches(same, k, 256, 4, 0);
  CHECK(!mixed_sizes(same, sb.data(), sb.size()));
  ErasureOptions o;
  CHECK(!o.ragged_rebuild);  // ships off
}

// The staging's arithmetic: survivor t of block b at k * off[b] + t * S[b],
// rebuilt shard r at e * off[b] + r * S[b]; the group's bytes are k * T and
// e * T with no padding.
TEST(staging_offsets, false) {
  const size_t k = 10, e = 2;
  const size_t sz[4] = {64, 4096, 0, 192}, off[5] = {0, 64, 4160, 4160, 4352};
  CHECK_EQ(batch_shard_offset(off[1], k, 0, sz[1]), 640);
  CHECK_EQ(batch_shard_offset(off[1], k, 9, sz[1]), 640 + 9 * 4096);
  CHECK_EQ(batch_shard_offset(off[3], k, 9, sz[3]) + sz[3], k * off[4]);
  CHECK_EQ(batch_shard_offset(off[3], e, 1, sz[3]) + sz[3], e * off[4]);
  CHECK_EQ(batch_shard_offset(off[1], e, 1, sz[1]), 2 * 64 + 4096);
}

// The device partition is the other ragged calls': ranges cut on block
// boundaries by bytes, each range's byte offset the sum of the sizes before.
TEST(device_split, false) {
  const std::vector<size_t> sz{64, 64, 4096, 0, 64, 8192, 64, 0, 0, 640, 64, 4096};
  for (size_t parts : {1, 2, 3, 4}) {
    const std::vector<size_t> cuts = cut_ragged_ranges(sz.data(), sz.size(), parts);
    CHECK(cuts.front() == 0 && cuts.back() == sz.size() && cuts.size() <= parts + 1);
    for (size_t i = 0; i + 1 < cuts.size(); ++i) CHECK(cuts[i + 1] > cuts[i]);
  }
}

// ------------------------------------------------------------- GPU tests
// Per-block patterns: m holders down, every block back bit-exact with the
// key on and off; with it on one ragged call per distinct e and exactly
// k * sum(S[b]) survivor bytes staged.
TEST(multi_fetch_ragged_on_and_off, true) {
  const std::vector<Block> bs = mixed_blocks();
  for (bool ragged : {true, false}) {
    Net net(16, 10, 4, ragged, 1 << 30);
    net.ec->store_many(bs);
    CHECK_EQ(take_down(net, 4), 4);
    std::set<int> es;
    size_t T = 0;
    for (auto& b : bs)
      if (const int e = net.lost_data(b.address, 10)) {
        es.insert(e);
        T += memo_ec_shard_size(b.data.size(), 10);
      }
    CHECK(es.size() >= 2);
    const uint64_t r0 = net.ec->codec().ragged_calls(), s0 = net.ec->codec().segments_calls();
    const uint64_t g0 = net.ec->ragged_rebuild_staged();
    CHECK_EQ(multi_fetch(net, bs), bs.size());
    if (ragged) {
      CHECK_EQ(net.ec->codec().ragged_calls() - r0, es.size());
      CHECK_EQ(net.ec->codec().segments_calls() - s0, 0);
      CHECK_EQ(net.ec->ragged_rebuild_staged() - g0, 10 * T);  // no padding byte
    } else {
      CHECK_EQ(net.ec->codec().ragged_calls() - r0, 0);
      CHECK_EQ(net.ec->codec().segments_calls() - s0, 1);
      CHECK_EQ(net.ec->ragged_rebuild_staged() - g0, 0);
    }
  }
}

// A repair after one node's eviction: every block that node held a shard of
// shares its pattern with the others that lost the same index.
TEST(repair_shared_patterns_ragged_on, true) {
  const std::vector<Block> bs = mixed_blocks();
  Net net(16, 10, 4, true, 2);
  net.ec->store_many(bs);
  std::shared_ptr<Node> victim;
  for (auto& n : net.nodes)
    if (!victim && !n->silo->list().empty()) victim = n;
  CHECK(victim != nullptr);
  net.overlay.set_up(victim->id, false);
  const uint64_t r0 = net.ec->codec().ragged_calls(), u0 = net.ec->codec().uniform_calls();
  const auto rep = net.ec->evict(victim->id);
  CHECK(rep.shards_rebuilt > 0);
  CHECK_EQ(rep.codec_calls, net.ec->codec().ragged_calls() - r0);  // the report counts every call
  CHECK_EQ(rep.unrecoverable, 0);
  CHECK(net.ec->codec().ragged_calls() > r0);
  CHECK(net.ec->codec().uniform_calls() > u0);  // shared patterns went ragged too
  for (auto& b : bs) CHECK(net.ec->fetch(b.address)->data == b.data);
  CHECK_EQ(multi_fetch(net, bs), bs.size());
}

// A batch of one shard size makes the rebuild_segments call it made before.
TEST(uniform_sizes_make_no_ragged_call, true) {
  std::vector<Block> bs;
  for (int i = 0; i < 12; ++i) bs.push_back(make_chb(random_bytes(70000, 8000 + i)));
  for (bool ragged : {true, false}) {
    Net net(16, 10, 4, ragged, 1 << 30);
    net.ec->store_many(bs);
    CHECK_EQ(take_down(net, 4), 4);
    const uint64_t s0 = net.ec->codec().segments_calls();
    CHECK_EQ(multi_fetch(net, bs), bs.size());
    CHECK_EQ(net.ec->codec().ragged_calls(), 0);
    CHECK_EQ(net.ec->codec().segments_calls() - s0, 1);
  }
}

// Codec::rebuild_ragged on one device and cut over "two" (the same GPU
// twice), against Codec::rebuild block by block; then a shared pattern.
TEST(codec_rebuild_ragged_matches_rebuild_per_block, true) {
  const int k = 10, m = 4, e = 2;
  const std::vector<size_t> sz{4032, 64, 4160, 8256, 64, 0, 192, 0, 64, 64, 64, 640, 4096};
  const size_t n = sz.size();
  std::vector<size_t> off(n + 1, 0);
  for (size_t b = 0; b < n; ++b) off[b + 1] = off[b] + sz[b];
  const size_t T = off.back();
  const Buffer surv = random_bytes(k * T, 43);
  std::mt19937_64 r(99);
  Buffer sidx(n * k), lidx(n * e);
  for (size_t b = 0; b < n; ++b) {
    std::vector<uint8_t> p(k + m);
    for (int i = 0; i < k + m; ++i) p[i] = (uint8_t)i;
    std::shuffle(p.begin(), p.end(), r);
    std::copy(p.begin(), p.begin() + e, lidx.begin() + b * e);
    std::copy(p.begin() + e, p.begin() + e + k, sidx.begin() + b * k);
  }
  Codec one(0, 1);
  Buffer want(e * T, 0), wantu(e * T, 0);
  for (size_t b = 0; b < n; ++b)
    if (sz[b]) {
      one.rebuild(k, m, sz[b], 1, sidx.data() + b * k, surv.data() + k * off[b], lidx.data() + b * e, e,
                  want.data() + e * off[b]);
      one.rebuild(k, m, sz[b], 1, sidx.data(), surv.data() + k * off[b], lidx.data(), e,
                  wantu.data() + e * off[b]);
    }
  Codec two(std::vector<int>{0, 0}, 1);
  CHECK_EQ(two.devices(), 2);
  for (Codec* c : {&one, &two}) {
    const uint64_t r0 = c->ragged_calls(), b0 = c->rebuild_calls(), u0 = c->uniform_calls();
    Buffer got(e * T, 0xA5);
    c->rebuild_ragged(k, m, n, sz.data(), sidx.data(), surv.data(), lidx.data(), e, false, got.data());
    CHECK(got == want);
    Buffer gotu(e * T, 0xA5);
    c->rebuild_ragged(k, m, n, sz.data(), sidx.data(), surv.data(), lidx.data(), e, true, gotu.data());
    CHECK(gotu == wantu);
    CHECK_EQ(c->ragged_calls() - r0, 2);
    CHECK_EQ(c->rebuild_calls() - b0, 1);
    CHECK_EQ(c->uniform_calls() - u0, 1);
  }
}

int main(int argc, char** argv) {
  bool cpu_only = false;
  const char* filter = nullptr;
  for (int i = 1; i < argc; ++i) {
    if (!std::strcmp(argv[i], "--cpu-only")) cpu_only = true;
    else filter = argv[i];
  }
  int run = 0, failed = 0;
  for (auto& t : tests()) {
    if (cpu_only && t.gpu) continue;
    if (filter && !std::strstr(t.name, filter)) continue;
    const int before = g_fail;
    std::printf("[ RUN  ] %s\n", t.name);
    std::fflush(stdout);
    try {
      t.fn();
    } catch (std::exception& e) {
      std::fprintf(stderr, "  uncaught: %s\n", e.what());
      ++g_fail;
    }
    ++run;
    const bool ok = g_fail == before;
    failed += !ok;
    std::printf("[ %s ] %s\n", ok ? " OK " : "FAIL", t.name);
  }
  std::printf("%d tests, %d failed\n", run, failed);
  return failed ? 1 : 0;
}
