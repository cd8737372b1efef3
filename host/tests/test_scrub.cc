// test_scrub.cc -- ErasureConsensus::scrub(): every block's k + m shards read
// and verified on the GPU (memo_ec_verify_batch), the shard the code names
// rewritten once the reassembled block passes its address, the rest handed to
// the k-subset recovery.  The CPU tests cover the verdict word's decoding and
// the report's arithmetic; the GPU ones run RS(10,4) on 16 in-process nodes.
// (The small harness and reframe_shard are restated from test_erasure.cc,
// which stays a program of its own.)
//   usage: test_scrub [--cpu-only] [filter]
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

void store(Consensus& c, const Block& b) { c.store(std::make_unique<Block>(b), STORE_INSERT, nullptr); }

Buffer random_bytes(size_t n, uint64_t seed) {
  std::mt19937_64 r(seed);
  Buffer b(n);
  for (auto& x : b) x = (uint8_t)r();
  return b;
}

// `nodes` nodes with memory silos on one overlay and an erasure consensus
// client over it; no automatic eviction.
struct Net {
  Overlay overlay;
  std::vector<std::shared_ptr<Node>> nodes;
  std::unique_ptr<ErasureConsensus> ec;
  ErasureOptions o;
  Net(int n, int k, int m) {
    for (int i = 0; i < n; ++i) {
      uint8_t id[32] = {0};
      id[0] = (uint8_t)(nodes.size() + 1);
      id[1] = 0x4d;
      nodes.push_back(overlay.add_node(Address(id, 0, false), make_shard_local(std::make_unique<MemorySilo>())));
    }
    o.k = k;
    o.m = m;
    o.eviction_delay_ms = -1;
    ec = std::make_unique<ErasureConsensus>(std::make_unique<ReplicationConsensus>(overlay, 3), overlay, o);
  }
  std::shared_ptr<Node> holder(const Address& a, int i) {
    for (auto& n : nodes)
      if (n->has(shard_key(a, i))) return n;
    return nullptr;
  }
};

// Shard i of `a` on whichever node holds it, re-framed with a valid header
// and CRC around `payload_xor`-damaged bytes: it passes every per-shard
// check but has the wrong bytes.
bool reframe_shard(Net& net, const Address& a, int i, uint8_t payload_xor) {
  const Key key = shard_key(a, i);
  auto n = net.holder(a, i);
  if (!n) return false;
  Buffer w = n->silo->get(key);
  const uint8_t* pay = nullptr;
  const ShardHeader h = decode_shard(w, &pay);
  Buffer bad(pay, pay + h.shard_size);
  for (size_t x = 0; x < bad.size(); x += 61) bad[x] ^= payload_xor;
  n->silo->set(key, encode_shard(h, bad.data(), i), false, true);
  return true;
}
// The stored payload of shard i of `a`.
Buffer shard_payload(Net& net, const Address& a, int i) {
  auto n = net.holder(a, i);
  if (!n) return {};
  Buffer w = n->silo->get(shard_key(a, i));
  const uint8_t* pay = nullptr;
  const ShardHeader h = decode_shard(w, &pay);
  return Buffer(pay, pay + h.shard_size);
}
uint64_t stat(ErasureConsensus& ec, const char* key) { return std::stoull(from_json(ec.stats())[key]); }

using Report = ErasureConsensus::ScrubReport;

}  // namespace

// ------------------------------------------------------------- CPU tests
TEST(verdict_word_decoding, false) {
  Verdict v = decode_verdict(0);
  CHECK(v.clean() && !v.located() && v.mask == 0 && v.shard == -1);
  v = decode_verdict(0xFu | (7u << 16));  // all four rows, data shard 7
  CHECK(!v.clean() && v.located() && v.mask == 0xF && v.shard == 7);
  v = decode_verdict(0x4u | (12u << 16));  // parity row 2 of RS(10,4): shard 12
  CHECK(v.located() && v.mask == 0x4 && v.shard == 12);
  v = decode_verdict(0x5u | ((uint32_t)MEMO_EC_VERDICT_UNLOCATED << 16));
  CHECK(!v.clean() && !v.located() && v.mask == 0x5 && v.shard == -1);
  v = decode_verdict(0xFFFFu | (79u << 16));  // the limits: m = 16, shard 79
  CHECK(v.mask == 0xFFFF && v.shard == 79);
  CHECK(MEMO_EC_VERDICT_MASK(0x00FF000Fu) == 0xF && MEMO_EC_VERDICT_SHARD(0x00FF000Fu) == 0xFF);
}

TEST(scrub_report_arithmetic, false) {
  Report a, b;
  CHECK(a.consistent(14));
  a.blocks_checked = 20;
  a.blocks_clean = 17;
  a.blocks_skipped = 1;
  a.mismatches = 2;
  a.shards_rewritten = 3;
  a.codec_calls = 3;
  CHECK(a.consistent(14));
  b.blocks_checked = 5;
  b.blocks_clean = 4;
  b.mismatches = 1;
  b.unrecoverable = 1;
  b.codec_calls = 1;
  CHECK(b.consistent(14));
  a += b;
  CHECK_EQ(a.blocks_checked, 25);
  CHECK_EQ(a.blocks_clean, 21);
  CHECK_EQ(a.blocks_skipped, 1);
  CHECK_EQ(a.mismatches, 3);
  CHECK_EQ(a.shards_rewritten, 3);
  CHECK_EQ(a.unrecoverable, 1);
  CHECK_EQ(a.codec_calls, 4);
  CHECK(a.consistent(14));
  Report c = a;
  c.blocks_clean += 1;  // a block counted twice
  CHECK(!c.consistent(14));
  c = a;
  c.unrecoverable = 4;  // more than mismatched
  CHECK(!c.consistent(14));
  c = b;
  c.shards_rewritten = 1;  // an unrecoverable block is not touched
  CHECK(!c.consistent(14));
}

// ------------------------------------------------------------- GPU tests
// 20 blocks of three sizes: every one clean, one verify call per shard size.
TEST(scrub_clean, true) {
  Net net(16, 10, 4);
  const size_t sizes[3] = {4096, 70000, 300000};
  for (int i = 0; i < 20; ++i) store(*net.ec, make_chb(random_bytes(sizes[i % 3], 100 + i)));
  const uint64_t verify0 = net.ec->codec().verify_calls();
  const Report r = net.ec->scrub();
  CHECK_EQ(r.blocks_checked, 20);
  CHECK_EQ(r.blocks_clean, 20);
  CHECK_EQ(r.blocks_skipped, 0);
  CHECK_EQ(r.mismatches, 0);
  CHECK_EQ(r.shards_rewritten, 0);
  CHECK_EQ(r.unrecoverable, 0);
  CHECK_EQ(r.codec_calls, 3);
  CHECK_EQ(net.ec->codec().verify_calls() - verify0, 3);
  CHECK(r.consistent(14));
  CHECK_EQ(stat(*net.ec, "scrubbed_blocks"), 20);
  CHECK_EQ(stat(*net.ec, "scrub_mismatches"), 0);
  // several chunks: the same answer
  Net small(16, 10, 4);
  small.o.stage_bytes = 1 << 20;
  small.ec.reset();
  small.ec = std::make_unique<ErasureConsensus>(std::make_unique<ReplicationConsensus>(small.overlay, 3),
                                                small.overlay, small.o);
  for (int i = 0; i < 9; ++i) store(*small.ec, make_chb(random_bytes(300000, 200 + i)));
  const Report s = small.ec->scrub();
  CHECK_EQ(s.blocks_clean, 9);
  CHECK(s.codec_calls >= 3);  // 9 x 420 KiB of shards in 1 MiB chunks
}

// The silent case: a wrong parity shard does not disturb a healthy fetch.
TEST(scrub_rewrites_reframed_parity_shard, true) {
  Net net(16, 10, 4);
  Block b = make_chb(random_bytes(70000, 1)), c = make_chb(random_bytes(70000, 2));
  store(*net.ec, b);
  store(*net.ec, c);
  const Buffer good = shard_payload(net, b.address, 12);
  CHECK(reframe_shard(net, b.address, 12, 0x5a));
  CHECK(shard_payload(net, b.address, 12) != good);
  CHECK(net.ec->fetch(b.address)->data == b.data);
  CHECK_EQ(stat(*net.ec, "subset_recoveries"), 0);
  Report r = net.ec->scrub();
  CHECK_EQ(r.blocks_checked, 2);
  CHECK_EQ(r.blocks_clean, 1);
  CHECK_EQ(r.mismatches, 1);
  CHECK_EQ(r.shards_rewritten, 1);
  CHECK_EQ(r.unrecoverable, 0);
  CHECK_EQ(r.codec_calls, 1);
  CHECK(shard_payload(net, b.address, 12) == good);
  CHECK_EQ(stat(*net.ec, "subset_recoveries"), 0);  // located: no blind search
  r = net.ec->scrub();
  CHECK_EQ(r.blocks_clean, 2);
  CHECK_EQ(r.mismatches, 0);
  // a degraded fetch now decodes from good parity whichever it takes
  auto d3 = net.holder(b.address, 3);
  CHECK(d3 != nullptr);
  net.overlay.set_up(d3->id, false);
  CHECK(net.ec->fetch(b.address)->data == b.data);
  CHECK_EQ(stat(*net.ec, "subset_recoveries"), 0);
  net.overlay.set_up(d3->id, true);
  // stats() follows the reports
  CHECK_EQ(stat(*net.ec, "scrubbed_blocks"), 4);
  CHECK_EQ(stat(*net.ec, "scrub_mismatches"), 1);
  CHECK_EQ(stat(*net.ec, "scrub_shards_rewritten"), 1);
  CHECK_EQ(stat(*net.ec, "scrub_unrecoverable"), 0);
  CHECK_EQ(stat(*net.ec, "corrupt_shards_rewritten"), 1);
}

TEST(scrub_rewrites_reframed_data_shard, true) {
  Net net(16, 10, 4);
  Block b = make_chb(random_bytes(300000, 3));
  store(*net.ec, b);
  const Buffer good = shard_payload(net, b.address, 4);
  CHECK(reframe_shard(net, b.address, 4, 0xc3));
  const Report r = net.ec->scrub();
  CHECK_EQ(r.mismatches, 1);
  CHECK_EQ(r.shards_rewritten, 1);
  CHECK_EQ(r.unrecoverable, 0);
  CHECK(shard_payload(net, b.address, 4) == good);
  CHECK_EQ(stat(*net.ec, "subset_recoveries"), 0);  // the code named the shard
  CHECK(net.ec->fetch(b.address)->data == b.data);
  CHECK_EQ(stat(*net.ec, "subset_recoveries"), 0);  // and the fetch needs no recovery
  CHECK_EQ(net.ec->scrub().blocks_clean, 1);
}

// Two wrong shards: no single shard explains them (with m = 4 rows, two wrong
// data shards never pass for one), so the k-subset recovery out-votes both.
// Data shards 0 and 1: the subset that drops both is the 42nd the recovery
// tries with every shard in hand, inside its verify-subsets = 64.
TEST(scrub_two_wrong_shards_fall_back_to_recover, true) {
  Net net(16, 10, 4);
  Block b = make_chb(random_bytes(70000, 4));
  store(*net.ec, b);
  const Buffer g0 = shard_payload(net, b.address, 0), g1 = shard_payload(net, b.address, 1);
  CHECK(reframe_shard(net, b.address, 0, 0x21));
  CHECK(reframe_shard(net, b.address, 1, 0x42));
  const Report r = net.ec->scrub();
  CHECK_EQ(r.mismatches, 1);
  CHECK_EQ(r.shards_rewritten, 2);
  CHECK_EQ(r.unrecoverable, 0);
  CHECK(stat(*net.ec, "subset_recoveries") == 1);
  CHECK(shard_payload(net, b.address, 0) == g0);
  CHECK(shard_payload(net, b.address, 1) == g1);
  CHECK_EQ(net.ec->scrub().blocks_clean, 1);
  CHECK_EQ(stat(*net.ec, "scrub_shards_rewritten"), 2);
}

// m + 1 wrong shards: every k-subset holds a wrong one.  Counted, nothing
// rewritten, and the other blocks of the scrub are still checked.
TEST(scrub_unrecoverable_block_is_left_alone, true) {
  Net net(16, 10, 4);
  Block a = make_chb(random_bytes(50000, 5)), b = make_chb(random_bytes(50000, 6)),
        c = make_chb(random_bytes(4096, 7));
  store(*net.ec, a);
  store(*net.ec, b);
  store(*net.ec, c);
  const int wrong[5] = {0, 2, 4, 11, 13};
  for (int i : wrong) CHECK(reframe_shard(net, b.address, i, 0x77));
  std::vector<Buffer> before;
  for (int i = 0; i < 14; ++i) before.push_back(shard_payload(net, b.address, i));
  const Report r = net.ec->scrub();
  CHECK_EQ(r.blocks_checked, 3);
  CHECK_EQ(r.blocks_clean, 2);
  CHECK_EQ(r.mismatches, 1);
  CHECK_EQ(r.unrecoverable, 1);
  CHECK_EQ(r.shards_rewritten, 0);
  CHECK(r.consistent(14));
  for (int i = 0; i < 14; ++i) CHECK(shard_payload(net, b.address, i) == before[i]);
  CHECK_EQ(stat(*net.ec, "scrub_unrecoverable"), 1);
  CHECK_EQ(stat(*net.ec, "corrupt_shards_rewritten"), 0);
}

// A block with a holder out of reach is repair()'s business.
TEST(scrub_skips_block_with_holder_down, true) {
  Net net(16, 10, 4);
  Block b = make_chb(random_bytes(70000, 8));
  store(*net.ec, b);
  auto h = net.holder(b.address, 12);
  CHECK(h != nullptr);
  CHECK(reframe_shard(net, b.address, 5, 0x18));  // not looked at while a shard is missing
  net.overlay.set_up(h->id, false);
  auto reads = [&] {
    int64_t f = 0;
    for (auto& n : net.nodes) f += n->fetches.load();
    return f;
  };
  const int64_t reads0 = reads();
  Report r = net.ec->scrub();
  CHECK_EQ(r.blocks_checked, 1);
  CHECK_EQ(r.blocks_skipped, 1);
  CHECK_EQ(r.mismatches, 0);
  CHECK_EQ(r.codec_calls, 0);
  CHECK_EQ(reads() - reads0, 0);  // skipped before any shard is asked for
  net.overlay.set_up(h->id, true);
  r = net.ec->scrub();
  CHECK_EQ(r.blocks_skipped, 0);
  CHECK_EQ(r.mismatches, 1);
  CHECK_EQ(r.shards_rewritten, 1);
}

// `only` restricts the scan to the listed blocks.
TEST(scrub_only_listed_blocks, true) {
  Net net(16, 10, 4);
  Block a = make_chb(random_bytes(70000, 9)), b = make_chb(random_bytes(70000, 10)),
        c = make_chb(random_bytes(4096, 11));
  store(*net.ec, a);
  store(*net.ec, b);
  store(*net.ec, c);
  CHECK(reframe_shard(net, a.address, 10, 0x33));
  CHECK(reframe_shard(net, b.address, 10, 0x33));
  Block never = make_chb(random_bytes(100, 12));  // not stored: not in the index
  const std::vector<Address> only{b.address, c.address, never.address};
  Report r = net.ec->scrub(&only);
  CHECK_EQ(r.blocks_checked, 2);
  CHECK_EQ(r.blocks_clean, 1);
  CHECK_EQ(r.mismatches, 1);
  CHECK_EQ(r.shards_rewritten, 1);
  CHECK_EQ(r.codec_calls, 2);  // two shard sizes
  const std::vector<Address> none;
  r = net.ec->scrub(&none);
  CHECK_EQ(r.blocks_checked, 0);
  r = net.ec->scrub();  // a's wrong parity is still there
  CHECK_EQ(r.blocks_checked, 3);
  CHECK_EQ(r.mismatches, 1);
  CHECK_EQ(r.shards_rewritten, 1);
  CHECK_EQ(stat(*net.ec, "scrubbed_blocks"), 5);
  CHECK_EQ(stat(*net.ec, "scrub_mismatches"), 2);
  CHECK_EQ(stat(*net.ec, "scrub_shards_rewritten"), 2);
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
