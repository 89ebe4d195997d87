// Self-test of the text record loader (records.cpp, mlr_text_*), built with ThreadSanitizer
// and with AddressSanitizer + UBSan by
// mlcomp_amd.build.build_runtime_selftest(main='records_text_selftest.cpp').  It writes text
// files (u16 and u32 tokens) whose tokens tell their record and position, opens good and
// corrupt ones, and drives the C API from one consumer thread the way the python
// TextRecordLoader does: several epochs with 1 and 8 threads, an epoch restarted half way,
// slots released out of order, a loader destroyed with batches in flight.  Checks: the four
// readers refuse each other's files, bad loader arguments are refused, every batch is within
// the token and the sequence budget and maximal by the greedy rule, a slot holds exactly the
// tokens, lengths, labels and record numbers of its sequences, every record appears once per
// epoch at world 1, sharded training ranks run equal step counts over disjoint records,
// evaluation keeps file order and every batch, and the stream does not depend on the thread
// count.  Exit status 0 = pass.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#include <vector>

extern "C" {
void* mlr_open(const char*);
void* mlr_seg_open(const char*);
void* mlr_clip_open(const char*);
void* mlr_text_open(const char*);
void mlr_close(void*);
void mlr_text_shape(void*, uint64_t*);
void* mlr_loader_create(void*, int, int, int, int, double, double, double, double, uint64_t, int, int, int, int,
                        int, int);
void* mlr_text_loader_create(void*, int, int, int, int, uint64_t, int, int, int, int, int);
int mlr_text_loader_set_slot(void*, int, int32_t*);
int mlr_loader_set_slot(void*, int, uint8_t*, int64_t*, int32_t*);
int64_t mlr_loader_start_epoch(void*, uint64_t);
int mlr_loader_next(void*, int64_t*);
void mlr_loader_release(void*, int);
void mlr_loader_destroy(void*);
}

namespace {

constexpr int N = 300, MAXLEN = 32, VOCAB = 50000, MAX_TOKENS = 96, MAX_SEQS = 8;

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                \
    }                                                              \
  } while (0)

struct Hdr {
  char magic[8];
  uint32_t h, w, c, lb;
  uint64_t count, rb;
  uint64_t total;   // text files; the image kinds keep K / kind / F here
  uint8_t res[16];
};
static_assert(sizeof(Hdr) == 64, "header layout");

struct Entry {
  uint64_t off;
  uint32_t len, t0;
  int32_t label;
  uint32_t zero;
};
static_assert(sizeof(Entry) == 24, "index entry layout");

int len_of(int i) { return 1 + (int)((i * 2654435761u >> 7) % MAXLEN); }
int tok_of(int i, int t) { return (i * 37 + t * 101) % VOCAB; }

// record i: len_of(i) tokens tok_of(i, t), type0_length len / 2, label 1000 + i; `edit`
// corrupts the index before it is written, `cut` bytes are left off the end
void write_text_file(const std::string& path, int token_bytes, void (*edit)(Hdr&, std::vector<Entry>&) = nullptr,
                     size_t cut = 0) {
  Hdr hdr{};
  std::memcpy(hdr.magic, "MLTXT001", 8);
  std::vector<Entry> index(N);
  uint64_t total = 0;
  for (int i = 0; i < N; ++i) {
    index[i] = Entry{total, (uint32_t)len_of(i), (uint32_t)len_of(i) / 2, 1000 + i, 0};
    total += (uint64_t)len_of(i);
  }
  hdr.h = MAXLEN; hdr.w = token_bytes == 2 ? VOCAB : 100000; hdr.c = (uint32_t)token_bytes; hdr.lb = 4;
  hdr.count = N; hdr.rb = 0; hdr.total = total;
  if (edit) edit(hdr, index);
  std::vector<uint8_t> body(sizeof(Hdr) + index.size() * sizeof(Entry) + total * token_bytes);
  std::memcpy(body.data(), &hdr, sizeof(Hdr));
  std::memcpy(body.data() + sizeof(Hdr), index.data(), index.size() * sizeof(Entry));
  uint8_t* t = body.data() + sizeof(Hdr) + index.size() * sizeof(Entry);
  for (int i = 0; i < N; ++i)
    for (int k = 0; k < len_of(i); ++k) {
      if (token_bytes == 2) {
        const uint16_t v = (uint16_t)tok_of(i, k);
        std::memcpy(t, &v, 2);
      } else {
        const uint32_t v = (uint32_t)tok_of(i, k);
        std::memcpy(t, &v, 4);
      }
      t += token_bytes;
    }
  FILE* f = std::fopen(path.c_str(), "wb");
  CHECK(f);
  std::fwrite(body.data(), 1, body.size() - cut, f);
  std::fclose(f);
}

// a 2x2x3 image file of one of the three image kinds
void write_image_file(const std::string& path, const char* magic) {
  FILE* f = std::fopen(path.c_str(), "wb");
  CHECK(f);
  Hdr hdr{};
  std::memcpy(hdr.magic, magic, 8);
  const bool seg = magic[2] == 'S', clip = magic[2] == 'V';
  const size_t tail = 4;   // a label, or a 2x2 one-plane mask
  hdr.h = 2; hdr.w = 2; hdr.c = 3; hdr.lb = 4; hdr.count = 4; hdr.rb = 12 + tail;
  if (seg || clip) { const uint32_t one = 1; std::memcpy(&hdr.total, &one, 4); }   // K = 1 / F = 1
  std::fwrite(&hdr, sizeof(hdr), 1, f);
  std::vector<uint8_t> rec(12 + tail, 1);
  for (int i = 0; i < 4; ++i) std::fwrite(rec.data(), 1, rec.size(), f);
  std::fclose(f);
}

size_t slot_ints(int max_tokens, int max_seqs) {
  return (((size_t)2 + 3 * max_seqs + max_tokens + 1) & ~(size_t)1) + 2 * (size_t)max_seqs;
}

struct Ring {
  std::vector<std::vector<int64_t>> buf;   // int64 storage keeps the slots 8-byte aligned
  Ring(void* L, int depth, int max_tokens, int max_seqs)
      : buf(depth, std::vector<int64_t>(slot_ints(max_tokens, max_seqs) / 2 + 1, -1)) {
    for (int i = 0; i < depth; ++i) CHECK(mlr_text_loader_set_slot(L, i, (int32_t*)buf[i].data()) == 0);
  }
  const int32_t* slot(int s) const { return (const int32_t*)buf[s].data(); }
};

// the record numbers of slot s after checking every field of the batch against the file
std::vector<int> check_batch(const Ring& r, int s, int max_tokens, int max_seqs) {
  const int32_t* p = r.slot(s);
  const int n = p[0], total = p[1];
  CHECK(n >= 1 && n <= max_seqs && total >= 1 && total <= max_tokens);
  const int32_t* ent = p + 2;
  const int32_t* tok = ent + 3 * max_seqs;
  const size_t ioff = ((size_t)2 + 3 * max_seqs + max_tokens + 1) & ~(size_t)1;
  std::vector<int> ids;
  int off = 0;
  for (int i = 0; i < n; ++i) {
    int64_t rec;
    std::memcpy(&rec, p + ioff + 2 * (size_t)i, 8);
    CHECK(rec >= 0 && rec < N);
    const int id = (int)rec, len = len_of(id);
    CHECK(ent[3 * i] == len && ent[3 * i + 1] == len / 2 && ent[3 * i + 2] == 1000 + id);
    for (int t = 0; t < len; ++t) CHECK(tok[off + t] == tok_of(id, t));
    off += len;
    ids.push_back(id);
  }
  CHECK(off == total);
  return ids;
}

using Epochs = std::vector<std::vector<std::vector<int>>>;   // [epoch][batch][record]

// one rank's batches for `epochs` epochs; abandon_at >= 0 restarts the next epoch after that
// many batches; `hold` keeps two slots and releases them newest first
Epochs run(void* file, int max_tokens, int max_seqs, int world, int rank, int threads, int epochs, int abandon_at,
           int slow_us, int train = 1, bool hold = false, uint64_t seed = 4321) {
  void* L = mlr_text_loader_create(file, max_tokens, max_seqs, MAXLEN, train, seed, rank, world, train, threads, 3);
  CHECK(L);
  Ring ring(L, 4, max_tokens, max_seqs);
  Epochs out;
  for (int e = 0; e < epochs; ++e) {
    const int64_t nb = mlr_loader_start_epoch(L, (uint64_t)e);
    CHECK(nb >= 1);
    std::vector<std::vector<int>> seen;
    int held = -1;
    for (int64_t b = 0; b < nb; ++b) {
      if (abandon_at >= 0 && b == abandon_at) break;
      int64_t bi = -1;
      const int s = mlr_loader_next(L, &bi);
      CHECK(s >= 0 && bi == b);
      seen.push_back(check_batch(ring, s, max_tokens, max_seqs));
      if (slow_us) std::this_thread::sleep_for(std::chrono::microseconds(slow_us));
      if (!hold) {
        mlr_loader_release(L, s);
      } else if (held < 0) {
        held = s;
      } else {   // two in hand: the newer goes back first
        mlr_loader_release(L, s);
        mlr_loader_release(L, held);
        held = -1;
      }
    }
    if (held >= 0) mlr_loader_release(L, held);
    int64_t bi;
    if (abandon_at < 0) CHECK(mlr_loader_next(L, &bi) == -1);
    out.push_back(seen);
  }
  mlr_loader_destroy(L);
  return out;
}

// budgets, and the greedy rule: a batch closes only when the next sequence of the rank's
// order would pass the token budget or it is full
void check_greedy(const std::vector<std::vector<int>>& batches, int max_tokens, int max_seqs) {
  for (size_t b = 0; b < batches.size(); ++b) {
    int tokens = 0;
    for (int id : batches[b]) tokens += len_of(id);
    CHECK((int)batches[b].size() <= max_seqs && tokens <= max_tokens);
    if (b + 1 < batches.size())
      CHECK((int)batches[b].size() == max_seqs || tokens + len_of(batches[b + 1][0]) > max_tokens);
  }
}

std::vector<int> flat(const std::vector<std::vector<int>>& batches) {
  std::vector<int> out;
  for (const auto& b : batches) out.insert(out.end(), b.begin(), b.end());
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const std::string p16 = dir + "/text_selftest_u16.mlrec", p32 = dir + "/text_selftest_u32.mlrec",
                    bad = dir + "/text_selftest_bad.mlrec";
  write_text_file(p16, 2);
  write_text_file(p32, 4);
  // the four readers refuse each other's files
  const char* magics[3] = {"MLREC001", "MLSEG001", "MLVID001"};
  void* (*opens[4])(const char*) = {mlr_open, mlr_seg_open, mlr_clip_open, mlr_text_open};
  for (int k = 0; k < 3; ++k) {
    write_image_file(bad, magics[k]);
    for (int o = 0; o < 4; ++o) {
      void* h = opens[o](bad.c_str());
      CHECK((h != nullptr) == (o == k));
      if (h) mlr_close(h);
    }
  }
  for (int o = 0; o < 3; ++o) CHECK(opens[o](p16.c_str()) == nullptr && opens[o](p32.c_str()) == nullptr);
  // corrupt text files
  write_text_file(bad, 2, nullptr, 5);                                                      // short file
  CHECK(mlr_text_open(bad.c_str()) == nullptr);
  write_text_file(bad, 2, [](Hdr&, std::vector<Entry>& ix) { ix[7].len = 0; });
  CHECK(mlr_text_open(bad.c_str()) == nullptr);
  write_text_file(bad, 2, [](Hdr&, std::vector<Entry>& ix) { ix[7].len = MAXLEN + 1; });
  CHECK(mlr_text_open(bad.c_str()) == nullptr);
  write_text_file(bad, 2, [](Hdr&, std::vector<Entry>& ix) { ix[7].t0 = ix[7].len + 1; });
  CHECK(mlr_text_open(bad.c_str()) == nullptr);
  write_text_file(bad, 2, [](Hdr& h, std::vector<Entry>& ix) { ix[N - 1].off = h.total - ix[N - 1].len + 1; });
  CHECK(mlr_text_open(bad.c_str()) == nullptr);
  write_text_file(bad, 2, [](Hdr&, std::vector<Entry>& ix) { ix[3].off = ~0ull - 2; });     // offset + length wraps
  CHECK(mlr_text_open(bad.c_str()) == nullptr);
  write_text_file(bad, 2, [](Hdr& h, std::vector<Entry>&) { h.count = 0; });
  CHECK(mlr_text_open(bad.c_str()) == nullptr);
  write_text_file(bad, 2, [](Hdr& h, std::vector<Entry>&) { h.count = ~0ull / 8; });         // count * 24 wraps
  CHECK(mlr_text_open(bad.c_str()) == nullptr);
  write_text_file(bad, 2, [](Hdr& h, std::vector<Entry>&) { h.w = 70000; });                 // u16 tokens, large vocab
  CHECK(mlr_text_open(bad.c_str()) == nullptr);
  write_text_file(bad, 2, [](Hdr& h, std::vector<Entry>&) { h.c = 3; });
  CHECK(mlr_text_open(bad.c_str()) == nullptr);

  for (const std::string& path : {p16, p32}) {
    void* f = mlr_text_open(path.c_str());
    CHECK(f);
    uint64_t shp[5];
    mlr_text_shape(f, shp);
    uint64_t total = 0;
    for (int i = 0; i < N; ++i) total += (uint64_t)len_of(i);
    CHECK(shp[0] == N && shp[1] == MAXLEN && shp[3] == (path == p16 ? 2u : 4u) && shp[4] == total);
    // loader arguments
    CHECK(mlr_loader_create(f, 4, 8, 8, 1, 0.5, 1.0, 0.75, 1.333, 1, 0, 1, 1, 0, 1, 4) == nullptr);
    CHECK(mlr_text_loader_create(f, MAX_TOKENS, MAX_SEQS, MAXLEN - 1, 1, 1, 0, 1, 1, 2, 3) == nullptr);   // a longer record
    CHECK(mlr_text_loader_create(f, MAXLEN - 1, MAX_SEQS, MAXLEN, 1, 1, 0, 1, 1, 2, 3) == nullptr);      // max_len > max_tokens
    CHECK(mlr_text_loader_create(f, MAX_TOKENS, 0, MAXLEN, 1, 1, 0, 1, 1, 2, 3) == nullptr);
    CHECK(mlr_text_loader_create(f, MAX_TOKENS, 1025, MAXLEN, 1, 1, 0, 1, 1, 2, 3) == nullptr);
    CHECK(mlr_text_loader_create(f, MAX_TOKENS, MAX_SEQS, MAXLEN, 1, 1, 2, 2, 1, 2, 3) == nullptr);      // rank >= world
    // determinism across thread counts and consumer speed; plan invariants
    const Epochs ref = run(f, MAX_TOKENS, MAX_SEQS, 1, 0, 1, 3, -1, 0);
    CHECK(run(f, MAX_TOKENS, MAX_SEQS, 1, 0, 8, 3, -1, 150) == ref);
    CHECK(run(f, MAX_TOKENS, MAX_SEQS, 1, 0, 8, 3, -1, 0, 1, true) == ref);   // slots released out of order
    for (const auto& ep : ref) {
      check_greedy(ep, MAX_TOKENS, MAX_SEQS);
      const std::vector<int> ids = flat(ep);
      CHECK((int)ids.size() == N && (int)std::set<int>(ids.begin(), ids.end()).size() == N);
    }
    CHECK(ref[0] != ref[1] && ref[1] != ref[2]);
    CHECK(run(f, MAX_TOKENS, MAX_SEQS, 1, 0, 8, 1, -1, 0, 1, false, 99) [0] != ref[0]);   // another seed
    // the sequence budget binds when the token budget is wide
    const Epochs wide = run(f, MAXLEN * 4, 3, 1, 0, 8, 1, -1, 0);
    check_greedy(wide[0], MAXLEN * 4, 3);
    CHECK((int)flat(wide[0]).size() == N);
    // evaluation: file order, every batch
    const Epochs ev = run(f, MAX_TOKENS, MAX_SEQS, 1, 0, 8, 1, -1, 0, 0);
    const std::vector<int> order = flat(ev[0]);
    CHECK((int)order.size() == N);
    for (int i = 0; i < N; ++i) CHECK(order[(size_t)i] == i);
    check_greedy(ev[0], MAX_TOKENS, MAX_SEQS);
    // sharding: training ranks run equal step counts over disjoint records; evaluation ranks
    // partition the file
    for (int world : {2, 3})
      for (int th : {1, 8}) {
        std::vector<Epochs> tr, evs;
        for (int r = 0; r < world; ++r) {
          tr.push_back(run(f, MAX_TOKENS, MAX_SEQS, world, r, th, 2, -1, 0));
          evs.push_back(run(f, MAX_TOKENS, MAX_SEQS, world, r, th, 1, -1, 0, 0));
        }
        for (size_t e = 0; e < 2; ++e) {
          std::set<int> all;
          size_t count = 0;
          for (int r = 0; r < world; ++r) {
            CHECK(tr[r][e].size() == tr[0][e].size());
            check_greedy(tr[r][e], MAX_TOKENS, MAX_SEQS);
            const std::vector<int> ids = flat(tr[r][e]);
            all.insert(ids.begin(), ids.end());
            count += ids.size();
          }
          CHECK(all.size() == count && count <= (size_t)N && count + (size_t)world * MAX_SEQS * 2 >= (size_t)N);
        }
        std::set<int> all;
        for (int r = 0; r < world; ++r) {
          const std::vector<int> ids = flat(evs[r][0]);
          for (size_t i = 0; i < ids.size(); ++i) CHECK(ids[i] == r + (int)i * world);
          all.insert(ids.begin(), ids.end());
        }
        CHECK((int)all.size() == N);
      }
    // start_epoch half way through an epoch restarts cleanly
    for (int th : {1, 8}) {
      const Epochs a = run(f, MAX_TOKENS, MAX_SEQS, 1, 0, th, 4, 2, 0);
      for (size_t e = 0; e < a.size(); ++e) {
        CHECK(a[e].size() == 2);
        if (e < ref.size()) CHECK(a[e][0] == ref[e][0] && a[e][1] == ref[e][1]);
      }
    }
    // destroy while the consumer still holds slots and the workers are filling the rest
    for (int th : {1, 8}) {
      void* L = mlr_text_loader_create(f, MAX_TOKENS, MAX_SEQS, MAXLEN, 1, 9, 0, 1, 1, th, 3);
      CHECK(L);
      {
        Ring ring(L, 3, MAX_TOKENS, MAX_SEQS);
        CHECK(mlr_loader_start_epoch(L, 0) >= 3);
        int64_t bi = -1;
        CHECK(mlr_loader_next(L, &bi) == 0 && bi == 0);
        CHECK(mlr_loader_next(L, &bi) == 1 && bi == 1);
        mlr_loader_destroy(L);   // joins the workers before the ring's buffers go away
      }
    }
    // a loader without its slots does not start, and its slots are not image slots
    void* L = mlr_text_loader_create(f, MAX_TOKENS, MAX_SEQS, MAXLEN, 1, 9, 0, 1, 1, 2, 3);
    CHECK(L && mlr_loader_start_epoch(L, 0) == -1);
    uint8_t img[8];
    int64_t lab[2];
    int32_t par[8];
    CHECK(mlr_loader_set_slot(L, 0, img, lab, par) == 0 && mlr_loader_start_epoch(L, 0) == -1);
    mlr_loader_destroy(L);
    mlr_close(f);
  }
  std::remove(p16.c_str());
  std::remove(p32.c_str());
  std::remove(bad.c_str());
  std::printf("records text selftest ok\n");
  return 0;
}
