// test_ragged.cc -- the ragged store path: a batch of several shard sizes
// encoded by ONE memo_ec_encode_ragged call, every block staged at its own
// shard size ("ragged-store"), and Codec::encode_ragged / verify_ragged.
// The CPU tests cover the device partition of a ragged batch and the offset
// arithmetic place_batch reads shards through; the GPU ones run RS(10,4) on
// 16 in-process nodes.  (The small harness is restated from test_scrub.cc.)
//   usage: test_ragged [--cpu-only] [filter]
#include <cstdio>
#include <cstring>
#include <random>

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

struct Net {
  Overlay overlay;
  std::vector<std::shared_ptr<Node>> nodes;
  std::unique_ptr<ErasureConsensus> ec;
  ErasureOptions o;
  Net(int n, int k, int m, bool ragged, size_t stage_bytes = kStageBytes, int batch_window_us = 200) {
    for (int i = 0; i < n; ++i) {
      uint8_t id[32] = {0};
      id[0] = (uint8_t)(nodes.size() + 1);
      id[1] = 0x4d;
      nodes.push_back(overlay.add_node(Address(id, 0, false), make_shard_local(std::make_unique<MemorySilo>())));
    }
    o.k = k;
    o.m = m;
    o.eviction_delay_ms = -1;
    o.ragged_store = ragged;
    o.stage_bytes = stage_bytes;
    o.batch_window_us = batch_window_us;
    ec = std::make_unique<ErasureConsensus>(std::make_unique<ReplicationConsensus>(overlay, 3), overlay, o);
  }
  int holders(const Address& a, int total) {
    int h = 0;
    for (auto& n : nodes)
      for (int i = 0; i < total; ++i)
        if (n->has(shard_key(a, i))) {
          ++h;
          break;
        }
    return h;
  }
};

// 40 blocks of 100 B .. 300 KiB, seeded.
std::vector<Block> mixed_blocks() {
  std::mt19937_64 r(0x6D656D6F);
  std::vector<Block> bs;
  for (int i = 0; i < 40; ++i) {
    const size_t B = 100 + (size_t)(r() % ((300u << 10) - 100 + 1));
    bs.push_back(make_chb(random_bytes(B, 7000 + i)));
  }
  return bs;
}

// store_many's chunks, restated: blocks are taken until a chunk holds
// stage_bytes of shards.  Per chunk: the sum of its shard sizes, its
// power-of-two size buckets and whether it holds several shard sizes.
struct Chunk {
  size_t T = 0;
  std::set<int> buckets;
  std::set<size_t> sizes;
};
int bucket_of(size_t S) {
  int b = 0;
  while (S > 64) {
    S >>= 1;
    ++b;
  }
  return b;
}
std::vector<Chunk> chunks_of(const std::vector<Block>& bs, int k, int m, size_t stage_bytes) {
  std::vector<Chunk> out;
  for (size_t b0 = 0, n0 = 0; b0 < bs.size(); b0 += n0) {
    size_t bytes = 0;
    Chunk c;
    for (n0 = 0; b0 + n0 < bs.size() && (n0 == 0 || bytes < stage_bytes); ++n0) {
      const size_t S = memo_ec_shard_size(bs[b0 + n0].data.size(), k);
      bytes += (size_t)(k + m) * S;
      c.T += S;
      c.buckets.insert(bucket_of(S));
      c.sizes.insert(S);
    }
    out.push_back(c);
  }
  return out;
}

void check_all_fetch(Net& net, const std::vector<Block>& bs) {
  for (auto& b : bs) {
    CHECK_EQ(net.holders(b.address, 14), 14);
    CHECK(net.ec->fetch(b.address)->data == b.data);
  }
}

}  // namespace

// ------------------------------------------------------------- CPU tests
TEST(ragged_ranges_cover_and_balance, false) {
  const std::vector<size_t> sz{64, 64, 4096, 0, 64, 8192, 64, 0, 0, 640, 64, 4096};
  size_t total = 0;
  for (size_t s : sz) total += s;
  for (size_t parts : {1, 2, 3, 4, 8, 20}) {
    const std::vector<size_t> cuts = cut_ragged_ranges(sz.data(), sz.size(), parts);
    CHECK(cuts.size() >= 2 && cuts.size() <= parts + 1);
    CHECK_EQ(cuts.front(), 0);
    CHECK_EQ(cuts.back(), sz.size());
    size_t acc = 0;
    for (size_t i = 0; i + 1 < cuts.size(); ++i) {
      CHECK(cuts[i + 1] > cuts[i]);  // no empty range, cut on block boundaries
      // a range ends with the first block that takes the bytes so far to its share
      for (size_t b = cuts[i]; b < cuts[i + 1]; ++b) acc += sz[b];
      if (i + 2 < cuts.size()) {
        CHECK(acc * parts >= total * (i + 1));
        CHECK((acc - sz[cuts[i + 1] - 1]) * parts < total * (i + 1) || cuts[i + 1] - cuts[i] == 1);
      }
    }
    CHECK_EQ(acc, total);
  }
  // equal sizes: the uniform partition
  const std::vector<size_t> eq(12, 4096);
  const std::vector<size_t> c3 = cut_ragged_ranges(eq.data(), eq.size(), 3);
  CHECK(c3 == (std::vector<size_t>{0, 4, 8, 12}));
  CHECK(cut_ragged_ranges(eq.data(), 0, 4) == (std::vector<size_t>{0}));
  const std::vector<size_t> zeros(5, 0);
  const std::vector<size_t> cz = cut_ragged_ranges(zeros.data(), zeros.size(), 2);
  CHECK(cz.front() == 0 && cz.back() == 5);
}

TEST(batch_shard_offsets, false) {
  // uniform slots are the offsets place_batch computed before: block i's
  // data shard j at (i * k + j) * S, parity shard r at (i * m + r) * S
  const size_t k = 10, m = 4, S = 4160;
  for (size_t i : {0, 1, 7})
    for (size_t j = 0; j < k; ++j) CHECK_EQ(batch_shard_offset(i * S, k, j, S), (i * k + j) * S);
  for (size_t i : {0, 1, 7})
    for (size_t r = 0; r < m; ++r) CHECK_EQ(batch_shard_offset(i * S, m, r, S), (i * m + r) * S);
  // ragged: sizes 64, 4096, 0, 192 -> off 0, 64, 4160, 4160
  const size_t sz[4] = {64, 4096, 0, 192}, off[4] = {0, 64, 4160, 4160};
  CHECK_EQ(batch_shard_offset(off[1], k, 0, sz[1]), 640);            // behind block 0's 10 x 64
  CHECK_EQ(batch_shard_offset(off[1], k, 9, sz[1]), 640 + 9 * 4096);
  CHECK_EQ(batch_shard_offset(off[3], k, 0, sz[3]), 640 + 40960);    // the empty block takes nothing
  CHECK_EQ(batch_shard_offset(off[3], m, 3, sz[3]), 4 * 4160 + 3 * 192);
  // the last shard ends where the buffer does: per * T
  CHECK_EQ(batch_shard_offset(off[3], k, 9, sz[3]) + sz[3], k * (64 + 4096 + 0 + 192));
  ErasureOptions o;
  CHECK(!o.ragged_store);  // ships off
}

// The seeded batch the GPU tests store: one chunk at the default stage_bytes,
// several at 1 MiB, every one of them with several shard sizes (so "a ragged
// call per staged chunk" is what those tests see) and several size buckets.
TEST(mixed_batch_chunks, false) {
  const std::vector<Block> bs = mixed_blocks();
  CHECK_EQ(bs.size(), 40);
  for (auto& b : bs) CHECK(b.data.size() >= 100 && b.data.size() <= (300u << 10));
  const std::vector<Chunk> one = chunks_of(bs, 10, 4, kStageBytes);
  CHECK_EQ(one.size(), 1);
  CHECK(one[0].buckets.size() >= 3);
  const std::vector<Chunk> many = chunks_of(bs, 10, 4, (size_t)1 << 20);
  CHECK(many.size() >= 3);
  size_t T = 0;
  for (auto& c : many) {
    CHECK(c.sizes.size() > 1);
    T += c.T;
  }
  CHECK_EQ(T, one[0].T);
}

// ------------------------------------------------------------- GPU tests
// One chunk, then several: a ragged call per staged chunk, no padding staged.
TEST(mixed_store_ragged_on, true) {
  const std::vector<Block> bs = mixed_blocks();
  for (size_t stage : {kStageBytes, (size_t)1 << 20}) {
    Net net(16, 10, 4, true, stage);
    const std::vector<Chunk> ch = chunks_of(bs, 10, 4, stage);
    CHECK(stage == kStageBytes ? ch.size() == 1 : ch.size() >= 3);
    size_t T = 0, mixed = 0;
    for (auto& c : ch) {
      T += c.T;
      mixed += c.sizes.size() > 1;
    }
    CHECK_EQ(mixed, ch.size());  // every chunk of this batch holds several sizes
    const uint64_t r0 = net.ec->codec().ragged_calls(), e0 = net.ec->codec().encode_calls();
    const uint64_t d0 = net.ec->store_data_bytes(), l0 = net.ec->arena_leased_bytes();
    net.ec->store_many(bs);
    CHECK_EQ(net.ec->codec().ragged_calls() - r0, ch.size());
    CHECK_EQ(net.ec->codec().encode_calls() - e0, ch.size());  // and no other encode
    CHECK_EQ(net.ec->store_data_bytes() - d0, 10 * T);          // k * sum of S[b]: no padding byte
    CHECK_EQ(net.ec->arena_leased_bytes() - l0, 14 * T);        // data + parity leases
    check_all_fetch(net, bs);
    // degraded: two holders down
    int down = 0;
    for (auto& n : net.nodes)
      if (down < 2 && !n->silo->list().empty()) {
        net.overlay.set_up(n->id, false);
        ++down;
      }
    CHECK_EQ(down, 2);
    for (auto& b : bs) CHECK(net.ec->fetch(b.address)->data == b.data);
  }
}

// The key off: the per-bucket calls, padded to each bucket's largest shard.
TEST(mixed_store_ragged_off, true) {
  const std::vector<Block> bs = mixed_blocks();
  for (size_t stage : {kStageBytes, (size_t)1 << 20}) {
    Net net(16, 10, 4, false, stage);
    const std::vector<Chunk> ch = chunks_of(bs, 10, 4, stage);
    size_t calls = 0, T = 0;
    for (auto& c : ch) {
      calls += c.buckets.size();
      T += c.T;
    }
    const uint64_t r0 = net.ec->codec().ragged_calls(), e0 = net.ec->codec().encode_calls();
    const uint64_t d0 = net.ec->store_data_bytes();
    net.ec->store_many(bs);
    CHECK_EQ(net.ec->codec().ragged_calls() - r0, 0);
    CHECK_EQ(net.ec->codec().encode_calls() - e0, calls);
    CHECK(net.ec->store_data_bytes() - d0 > 10 * T);  // padding staged
    check_all_fetch(net, bs);
  }
}

// A batch of one shard size makes the uniform call either way.
TEST(uniform_batch_makes_no_ragged_call, true) {
  std::vector<Block> bs;
  for (int i = 0; i < 12; ++i) bs.push_back(make_chb(random_bytes(70000, 8000 + i)));
  for (bool ragged : {true, false}) {
    Net net(16, 10, 4, ragged);
    const uint64_t e0 = net.ec->codec().encode_calls();
    net.ec->store_many(bs);
    CHECK_EQ(net.ec->codec().ragged_calls(), 0);
    CHECK_EQ(net.ec->codec().encode_calls() - e0, 1);
    CHECK_EQ(net.ec->store_data_bytes(), 12 * 10 * memo_ec_shard_size(70000, 10));
    check_all_fetch(net, bs);
  }
}

// Concurrent single stores of several sizes meet in the batcher.
TEST(batcher_mixed_sizes, true) {
  Net net(16, 10, 4, true, kStageBytes, 20000);
  const std::vector<Block> bs = mixed_blocks();
  std::vector<std::thread> ts;
  for (int t = 0; t < 8; ++t)
    ts.emplace_back([&, t] {
      for (size_t i = t; i < bs.size(); i += 8) net.ec->store(std::make_unique<Block>(bs[i]), STORE_INSERT, nullptr);
    });
  for (auto& t : ts) t.join();
  CHECK(net.ec->codec().encode_calls() < bs.size());  // batched
  CHECK(net.ec->codec().ragged_calls() >= 1);
  check_all_fetch(net, bs);
}

// Codec::encode_ragged / verify_ragged: one device, and the block range cut
// over "two" (the same GPU twice), against the uniform call block by block.
TEST(codec_ragged_matches_uniform_per_block, true) {
  const int k = 10, m = 4;
  const std::vector<size_t> sz{4032, 64, 4160, 8256, 64, 0, 192, 0, 64, 64, 64, 640, 4096};
  std::vector<size_t> off(sz.size() + 1, 0);
  for (size_t b = 0; b < sz.size(); ++b) off[b + 1] = off[b] + sz[b];
  const size_t T = off.back();
  const Buffer data = random_bytes(k * T, 42);
  Codec one(0, 1);
  Buffer want(m * T, 0);
  for (size_t b = 0; b < sz.size(); ++b)
    if (sz[b]) one.encode(k, m, sz[b], 1, data.data() + k * off[b], want.data() + m * off[b]);
  const uint64_t e0 = one.encode_calls();
  Buffer got(m * T, 0xA5);
  one.encode_ragged(k, m, sz.size(), sz.data(), data.data(), got.data());
  CHECK(got == want);
  CHECK_EQ(one.ragged_calls(), 1);
  CHECK_EQ(one.encode_calls() - e0, 1);
  Codec two(std::vector<int>{0, 0}, 1);
  CHECK_EQ(two.devices(), 2);
  Buffer got2(m * T, 0xA5);
  two.encode_ragged(k, m, sz.size(), sz.data(), data.data(), got2.data());
  CHECK(got2 == want);
  // verify: clean, then one wrong byte in block 3's parity shard 2 and one
  // in block 11's data shard 5
  std::vector<uint32_t> v(sz.size(), 0xFFFFFFFFu);
  two.verify_ragged(k, m, sz.size(), sz.data(), data.data(), want.data(), v.data());
  for (uint32_t w : v) CHECK_EQ(w, 0);
  Buffer d2 = data, p2 = want;
  p2[batch_shard_offset(off[3], m, 2, sz[3]) + 8255] ^= 0x40;
  d2[batch_shard_offset(off[11], k, 5, sz[11])] ^= 0x01;
  for (Codec* c : {&one, &two}) {
    std::fill(v.begin(), v.end(), 0xFFFFFFFFu);
    c->verify_ragged(k, m, sz.size(), sz.data(), d2.data(), p2.data(), v.data());
    for (size_t b = 0; b < sz.size(); ++b) {
      const Verdict x = decode_verdict(v[b]);
      if (b == 3) CHECK(x.mask == 0x4 && x.shard == 12);
      else if (b == 11) CHECK(x.mask == 0xF && x.shard == 5);
      else CHECK(x.clean());
    }
  }
  CHECK_EQ(two.ragged_calls(), 3);
  CHECK_EQ(two.verify_calls(), 2);
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
