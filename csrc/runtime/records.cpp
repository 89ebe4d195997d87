// mlcomp_amd native input pipeline: record files + a threaded batch gatherer.
//
// The reference feeds Catalyst from a PyTorch DataLoader (python workers decoding images,
// `mlcomp/contrib/dataset/classify.py:16-138`).  At ~11.5k img/s per MI355X (92k img/s per
// 8-GPU node) a python pipeline is the bottleneck, so the MI355X design splits the work:
//   * host (this file): a memory-mapped record file of fixed-size uint8 HWC images + int32
//     labels; per epoch a seeded global shuffle, sharded by rank; worker threads copy the
//     raw records of a batch into a caller-owned (pinned) slot and draw the per-sample
//     augmentation parameters (RandomResizedCrop box + horizontal flip, or the centre crop
//     for evaluation) from a counter-based RNG keyed by (seed, epoch, sample);
//   * device (csrc/kernels/augment.hip): one kernel crops, bilinearly resizes, flips,
//     normalises and writes the layout the model's first layer reads (the native stem's
//     space-to-depth image), so the host never touches a float and PCIe carries uint8.
//
// File format (".mlrec", little endian): 64-byte header
//   char magic[8] = "MLREC001"; u32 H, W, C; u32 label_bytes (= 4); u64 count;
//   u64 record_bytes (= H*W*C + 4); u8 reserved[24]
// followed by `count` records {u8 image[H][W][C]; i32 label}.
//
// Segmentation files carry a mask instead of a label: magic "MLSEG001", label_bytes =
// H*W*K, record_bytes = H*W*(C+K), reserved[0..3] = u32 K (mask planes, 1..4),
// reserved[4..7] = u32 kind (0: planes, a pixel is foreground for plane k iff its byte is
// non-zero; 1: index, K = 1 and the byte is the class id); records
// {u8 image[H][W][C]; u8 mask[H][W][K]}.  The other magic keeps either reader from
// opening the other kind of file.  The segmentation loader (mlr_seg_*) is the same slot
// state machine with a mask buffer in place of the labels and params[batch][8] =
// {y0, x0, h, w, hflip, vflip, transpose, 0}: the box draws are the classification ones,
// then three independent coins that span the eight symmetries of the square.
//
// Video clip files: magic "MLVID001", label_bytes = 4, record_bytes = F*H*W*C + 4,
// reserved[0..3] = u32 F (frames per record, >= 1, fixed per file); records
// {u8 frames[F][H][W][C]; i32 label}.  The clip loader (mlr_clip_*) has a clip length T and
// a frame stride s with span = (T-1)*s + 1 <= F.  It draws the box and the flip exactly as
// the classification loader does (one transform for every frame of a clip), then the first
// frame t0 = r % (F - span + 1) (evaluation: the centre, (F - span) / 2);
// params[batch][8] = {y0, x0, h, w, flip, t0, s, 0}.  The gather threads copy only the T
// frames t0 + k*s, so a slot's image buffer is [batch][T][H][W][C].
//
// Text files: magic "MLTXT001", H = the longest record in tokens, W = vocab_size, C =
// token_bytes (2: u16, only for vocab <= 65536; 4: u32), label_bytes = 4, record_bytes = 0
// (records vary in length), reserved[0..7] = u64 total_tokens.  After the header come
// `count` index entries {u64 token_offset; u32 length; u32 type0_length; i32 label; u32 zero}
// (tokens [0, type0_length) of a record have token type 0, the rest type 1), then
// total_tokens tokens.  mlr_text_open checks every entry.  The text loader (mlr_text_*) runs
// the same slot state machine, but a batch is a token budget: start_epoch plans the epoch
// (seeded order, rank r takes every world-th entry without padding, batches filled greedily
// until the next sequence would pass max_tokens or the batch holds max_seqs; in training all
// ranks run the step count of the rank with the fewest) and the gather threads write
// sequences at the offsets of the plan.  A slot is one int32 buffer, so a batch crosses PCIe
// in one copy: {nseq, total}, {length, type0_length, label}[max_seqs], tokens[max_tokens]
// widened to int32, then (8-byte aligned, host only) int64 indices[max_seqs].  Rows past
// `total` and entries past `nseq` keep whatever an earlier batch left there.
//
// Slot protocol: the caller registers `depth` slots (image buffer of batch*H*W*C bytes,
// int64 labels[batch], int32 params[batch][5]); next() blocks until the next batch of the
// epoch (in order) is complete and returns its slot, release(slot) hands it back.  Batches
// are split into chunks of samples so every worker thread helps fill the batch the
// consumer waits for.  All shared state is guarded by one mutex; the copies run unlocked.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <numeric>
#include <thread>
#include <vector>

namespace {

constexpr char MAGIC[8] = {'M', 'L', 'R', 'E', 'C', '0', '0', '1'};
constexpr char SEG_MAGIC[8] = {'M', 'L', 'S', 'E', 'G', '0', '0', '1'};
constexpr char CLIP_MAGIC[8] = {'M', 'L', 'V', 'I', 'D', '0', '0', '1'};
constexpr char TEXT_MAGIC[8] = {'M', 'L', 'T', 'X', 'T', '0', '0', '1'};

enum Kind { LABELS = 0, SEG = 1, CLIP = 2, TEXT = 3 };   // what a record holds next to its image(s)

struct Header {
  char magic[8];
  uint32_t H, W, C, label_bytes;
  uint64_t count, record_bytes;
  uint8_t reserved[24];
};
static_assert(sizeof(Header) == 64, "header layout");

struct TextEntry {   // one index entry of a text file
  uint64_t token_offset;
  uint32_t length, type0_length;
  int32_t label;
  uint32_t zero;
};
static_assert(sizeof(TextEntry) == 24, "index entry layout");

struct RecordFile {
  int fd = -1;
  const uint8_t* map = nullptr;
  size_t size = 0;
  Header h{};
  uint32_t K = 0, kind = 0;   // mask planes and kind of a segmentation file (K = 0: labels)
  uint32_t F = 0;             // frames per record of a clip file (0: not a clip file)
  const TextEntry* index = nullptr;   // text file: `count` entries, then the tokens
  const uint8_t* tokens = nullptr;
  uint64_t total_tokens = 0;
  Kind what() const { return index ? TEXT : F ? CLIP : K ? SEG : LABELS; }
  const uint8_t* record(uint64_t i) const { return map + sizeof(Header) + i * h.record_bytes; }
};

// counter-based RNG: splitmix64 of a key, so a sample's augmentation depends only on
// (seed, epoch, sample index) - not on thread scheduling
inline uint64_t mix(uint64_t z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
struct Rng {
  uint64_t s;
  explicit Rng(uint64_t key) : s(mix(key)) {}
  uint64_t next() { return s = mix(s); }
  double uniform() { return (next() >> 11) * (1.0 / 9007199254740992.0); }
};

enum SlotState { FREE = 0, FILLING = 1, READY = 2, INUSE = 3 };

struct Slot {
  uint8_t* img = nullptr;
  int64_t* lab = nullptr;    // classification
  uint8_t* mask = nullptr;   // segmentation
  int32_t* par = nullptr;
  int32_t* txt = nullptr;    // text: the whole slot
  SlotState state = FREE;
  int64_t batch = -1;
  int remaining = 0;   // chunks still being filled
};

struct Loader {
  const RecordFile* rf;
  int batch, out_h, out_w, train;
  double smin, smax, rmin, rmax;
  uint64_t seed;
  int rank, world, shuffle, drop_last;
  int chunk = 16;
  bool seg = false;   // image + mask records, params[batch][8]
  bool clip = false;  // clip records: clip_len frames at frame_stride, params[batch][8]
  int clip_len = 0, frame_stride = 1;
  bool text = false;  // token-budget batches: `batch` is max_seqs, a batch's rows come from the plan
  int max_tokens = 0;
  std::vector<uint64_t> bstart;   // text: batch b holds order[bstart[b] .. bstart[b+1])
  std::vector<int32_t> doff;      // text: token offset of order[k] inside its batch
  std::vector<Slot> slots;
  // epoch
  uint64_t epoch = 0;
  std::vector<uint64_t> order;   // this rank's samples, padded to a whole number of batches
  int64_t nbatches = 0, nitems = 0, next_item = 0, consume_next = 0;
  int filling = 0;               // chunks being copied right now
  bool started = false, stop = false;
  std::mutex mu;
  std::condition_variable cv_work, cv_ready, cv_idle;
  std::vector<std::thread> workers;

  int chunks_per_batch() const { return (batch + chunk - 1) / chunk; }

  int par_stride() const { return seg || clip ? 8 : 5; }
  int span() const { return (clip_len - 1) * frame_stride + 1; }

  // one sample's augmentation: the source box {y0, x0, h, w}, then {flip}, for
  // segmentation {hflip, vflip, transpose, 0}, for clips {flip, t0, frame stride, 0}
  void params(uint64_t sample, int32_t* p) const {
    const int H = (int)rf->h.H, W = (int)rf->h.W;
    Rng g(seed * 0x100000001b3ull ^ (epoch << 40) ^ sample);
    for (int i = 4; i < par_stride(); ++i) p[i] = 0;
    if (!train) {   // centre crop of the output size (whole image if it is smaller)
      const int h = std::min(H, out_h), w = std::min(W, out_w);
      p[0] = (H - h) / 2; p[1] = (W - w) / 2; p[2] = h; p[3] = w;
      if (clip) { p[5] = ((int)rf->F - span()) / 2; p[6] = frame_stride; }
      return;
    }
    draw_box(g, H, W, p);
    const int coins = seg ? 3 : 1;
    for (int i = 0; i < coins; ++i) p[4 + i] = (int)(g.next() & 1);
    if (clip) {   // after the classification draws, so the box and the flip are the image loader's
      p[5] = (int)(g.next() % (uint64_t)((int)rf->F - span() + 1));
      p[6] = frame_stride;
    }
  }

  void draw_box(Rng& g, int H, int W, int32_t* p) const {
    const double area = (double)H * W;
    for (int attempt = 0; attempt < 10; ++attempt) {   // torchvision RandomResizedCrop
      const double a = area * (smin + (smax - smin) * g.uniform());
      const double lr = std::log(rmin) + (std::log(rmax) - std::log(rmin)) * g.uniform();
      const double r = std::exp(lr);
      const int w = (int)std::lround(std::sqrt(a * r)), h = (int)std::lround(std::sqrt(a / r));
      if (w > 0 && h > 0 && w <= W && h <= H) {
        p[0] = (int)(g.next() % (uint64_t)(H - h + 1));
        p[1] = (int)(g.next() % (uint64_t)(W - w + 1));
        p[2] = h; p[3] = w;
        return;
      }
    }
    const int s = std::min(H, W);   // fallback: centre square
    p[0] = (H - s) / 2; p[1] = (W - s) / 2; p[2] = s; p[3] = s;
  }

  size_t text_index_off() const { return ((size_t)2 + 3 * (size_t)batch + (size_t)max_tokens + 1) & ~(size_t)1; }

  // greedy token-budget batches over `ord`, the rule of TokenBudgetBatchSampler._fill:
  // starts[k] is the position of batch k's first sequence, the last entry ord.size()
  void plan_batches(const std::vector<uint64_t>& ord, std::vector<uint64_t>& starts) const {
    starts.assign(1, 0);
    int n = 0;
    int64_t tokens = 0;
    for (size_t k = 0; k < ord.size(); ++k) {
      const int64_t len = rf->index[ord[k]].length;
      if (n && (tokens + len > max_tokens || n == batch)) {
        starts.push_back(k);
        n = 0;
        tokens = 0;
      }
      ++n;
      tokens += len;
    }
    if (n) starts.push_back(ord.size());
  }

  // this rank's share of the epoch order `all` and its batches (see the file comment)
  void plan_text(const std::vector<uint64_t>& all) {
    std::vector<uint64_t> mine, other, starts;
    size_t steps = SIZE_MAX;
    for (int r = 0; r < world; ++r) {
      if (r != rank && !train) continue;   // evaluation: all of this rank's own batches
      std::vector<uint64_t>& ord = r == rank ? mine : other;
      ord.clear();
      for (size_t i = (size_t)r; i < all.size(); i += (size_t)world) ord.push_back(all[i]);
      plan_batches(ord, starts);
      steps = std::min(steps, starts.size() - 1);
      if (r == rank) bstart = starts;
    }
    bstart.resize(steps + 1);
    mine.resize((size_t)bstart[steps]);
    order = mine;
    doff.assign(order.size(), 0);
    for (size_t b = 0; b < steps; ++b) {
      int32_t off = 0;
      for (uint64_t k = bstart[b]; k < bstart[b + 1]; ++k) {
        doff[(size_t)k] = off;
        off += (int32_t)rf->index[order[(size_t)k]].length;
      }
    }
    nbatches = (int64_t)steps;
  }

  void fill_text(Slot& sl, int64_t b, int c) {
    const uint64_t p0 = bstart[(size_t)b], p1 = bstart[(size_t)b + 1];
    const int n = (int)(p1 - p0);
    int32_t* ent = sl.txt + 2;
    int32_t* tok = ent + 3 * (size_t)batch;
    int32_t* idx = sl.txt + text_index_off();
    if (c == 0) {
      sl.txt[0] = n;
      sl.txt[1] = doff[(size_t)p1 - 1] + (int32_t)rf->index[order[(size_t)p1 - 1]].length;
    }
    const int i0 = c * chunk, i1 = std::min(n, i0 + chunk);
    for (int i = i0; i < i1; ++i) {
      const uint64_t s = order[(size_t)p0 + i];
      const TextEntry& e = rf->index[s];
      ent[3 * i] = (int32_t)e.length; ent[3 * i + 1] = (int32_t)e.type0_length; ent[3 * i + 2] = e.label;
      int32_t* dst = tok + doff[(size_t)p0 + i];
      if (rf->h.C == 2) {
        const uint16_t* src = (const uint16_t*)rf->tokens + e.token_offset;
        for (uint32_t t = 0; t < e.length; ++t) dst[t] = (int32_t)src[t];
      } else {
        std::memcpy(dst, (const uint32_t*)rf->tokens + e.token_offset, (size_t)e.length * 4);
      }
      const int64_t rec = (int64_t)s;
      std::memcpy(idx + 2 * (size_t)i, &rec, 8);
    }
  }

  void fill(Slot& sl, int64_t b, int c) {
    if (text) return fill_text(sl, b, c);
    const size_t ib = (size_t)rf->h.H * rf->h.W * rf->h.C;
    const size_t mb = (size_t)rf->h.H * rf->h.W * rf->K;
    const int i0 = c * chunk, i1 = std::min(batch, i0 + chunk);
    for (int i = i0; i < i1; ++i) {
      const uint64_t s = order[(size_t)b * batch + i];
      const uint8_t* rec = rf->record(s);
      if (clip) {   // only the selected frames t0 + k*stride cross into the slot
        int32_t* p = sl.par + par_stride() * i;
        params(s, p);
        for (int k = 0; k < clip_len; ++k)
          std::memcpy(sl.img + ((size_t)i * clip_len + k) * ib, rec + (size_t)(p[5] + k * p[6]) * ib, ib);
        int32_t lab;
        std::memcpy(&lab, rec + (size_t)rf->F * ib, 4);
        sl.lab[i] = lab;
        continue;
      }
      std::memcpy(sl.img + (size_t)i * ib, rec, ib);
      if (seg) {
        std::memcpy(sl.mask + (size_t)i * mb, rec + ib, mb);
      } else {
        int32_t lab;
        std::memcpy(&lab, rec + ib, 4);
        sl.lab[i] = lab;
      }
      params(s, sl.par + par_stride() * i);
    }
  }

  void worker() {
    std::unique_lock<std::mutex> lk(mu);
    for (;;) {
      cv_work.wait(lk, [&] { return stop || (started && next_item < nitems); });
      if (stop) return;
      const int64_t item = next_item;
      const int64_t b = item / chunks_per_batch();
      const int c = (int)(item % chunks_per_batch());
      Slot& sl = slots[(size_t)(b % (int64_t)slots.size())];
      if (!(sl.batch == b && sl.state == FILLING) && sl.state != FREE) {
        // the slot still holds an older batch: wait for the consumer to release it
        cv_work.wait(lk, [&] { return stop || !started || next_item != item || sl.state == FREE ||
                                      (sl.batch == b && sl.state == FILLING); });
        continue;
      }
      if (sl.state == FREE) { sl.state = FILLING; sl.batch = b; sl.remaining = chunks_per_batch(); }
      ++next_item;
      ++filling;
      lk.unlock();
      fill(sl, b, c);
      lk.lock();
      --filling;
      if (--sl.remaining == 0) { sl.state = READY; cv_ready.notify_all(); }
      if (filling == 0) cv_idle.notify_all();
      cv_work.notify_all();
    }
  }

  void start_epoch(uint64_t e) {
    std::unique_lock<std::mutex> lk(mu);
    // stop claiming new work of the old epoch, let the copies in flight finish
    next_item = nitems;
    cv_idle.wait(lk, [&] { return filling == 0; });
    for (auto& s : slots) { s.state = FREE; s.batch = -1; s.remaining = 0; }
    epoch = e;
    const uint64_t n = rf->h.count;
    std::vector<uint64_t> all(n);
    std::iota(all.begin(), all.end(), 0ull);
    if (shuffle) {   // Fisher-Yates with the epoch's RNG: identical on every rank
      Rng g(seed ^ 0x5851f42d4c957f2dull ^ (e * 0x2545f4914f6cdd1dull));
      for (uint64_t i = n; i > 1; --i) std::swap(all[i - 1], all[g.next() % i]);
    }
    if (text) {
      plan_text(all);
      nitems = nbatches * chunks_per_batch();
      next_item = 0;
      consume_next = 0;
      started = true;
      cv_work.notify_all();
      return;
    }
    // shard: pad to a multiple of world (wrapping), rank takes every world-th sample
    const uint64_t per = (n + world - 1) / world;
    order.clear();
    for (uint64_t i = 0; i < per; ++i) order.push_back(all[(i * world + rank) % n]);
    const uint64_t nb = drop_last ? per / batch : (per + batch - 1) / batch;
    // a last partial batch is filled up by wrapping around this rank's samples (fixed slot
    // shape); RecordLoader.real_rows() tells the consumer how many rows are real
    for (uint64_t i = order.size(); i < nb * batch; ++i) order.push_back(order[i % per]);
    nbatches = (int64_t)nb;
    nitems = nbatches * chunks_per_batch();
    next_item = 0;
    consume_next = 0;
    started = true;
    cv_work.notify_all();
  }

  int next(int64_t* batch_index) {
    std::unique_lock<std::mutex> lk(mu);
    if (!started || consume_next >= nbatches) return -1;
    const int64_t b = consume_next;
    Slot& sl = slots[(size_t)(b % (int64_t)slots.size())];
    cv_ready.wait(lk, [&] { return stop || (sl.batch == b && sl.state == READY); });
    if (stop) return -1;
    sl.state = INUSE;
    ++consume_next;
    if (batch_index) *batch_index = b;
    return (int)(b % (int64_t)slots.size());
  }

  void release(int s) {
    std::lock_guard<std::mutex> lk(mu);
    if (s < 0 || s >= (int)slots.size() || slots[(size_t)s].state != INUSE) return;
    slots[(size_t)s].state = FREE;
    slots[(size_t)s].batch = -1;
    cv_work.notify_all();
  }

  ~Loader() {
    {
      std::lock_guard<std::mutex> lk(mu);
      stop = true;
    }
    cv_work.notify_all();
    cv_ready.notify_all();
    for (auto& t : workers) t.join();
  }
};

}  // namespace

#define MLR_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

// the checks of a text file: header, sizes and every index entry
bool open_text(RecordFile* rf) {
  const Header& h = rf->h;
  if (std::memcmp(h.magic, TEXT_MAGIC, 8) != 0 || h.count == 0 || h.label_bytes != 4 || h.record_bytes != 0) return false;
  if (h.H == 0 || h.W == 0 || !(h.C == 4 || (h.C == 2 && h.W <= 65536))) return false;
  uint64_t total;
  std::memcpy(&total, h.reserved, 8);
  const uint64_t body = rf->size - sizeof(Header);
  if (h.count > body / sizeof(TextEntry)) return false;
  if (total > (body - h.count * sizeof(TextEntry)) / h.C) return false;
  const auto* index = (const TextEntry*)(rf->map + sizeof(Header));
  for (uint64_t i = 0; i < h.count; ++i) {
    const TextEntry& e = index[i];
    if (e.length < 1 || e.length > h.H || e.type0_length > e.length || e.token_offset > total ||
        e.length > total - e.token_offset)
      return false;
  }
  rf->index = index;
  rf->tokens = rf->map + sizeof(Header) + h.count * sizeof(TextEntry);
  rf->total_tokens = total;
  return true;
}

RecordFile* open_file(const char* path, Kind kind) {
  auto* rf = new RecordFile();
  rf->fd = open(path, O_RDONLY);
  struct stat st{};
  if (rf->fd < 0 || fstat(rf->fd, &st) != 0 || (size_t)st.st_size < sizeof(Header)) {
    if (rf->fd >= 0) close(rf->fd);
    delete rf;
    return nullptr;
  }
  rf->size = (size_t)st.st_size;
  void* m = mmap(nullptr, rf->size, PROT_READ, MAP_SHARED, rf->fd, 0);
  if (m == MAP_FAILED) { close(rf->fd); delete rf; return nullptr; }
  rf->map = (const uint8_t*)m;
  std::memcpy(&rf->h, rf->map, sizeof(Header));
  if (kind == TEXT) {
    if (open_text(rf)) return rf;
    munmap(m, rf->size);
    close(rf->fd);
    delete rf;
    return nullptr;
  }
  const uint64_t need = sizeof(Header) + rf->h.count * rf->h.record_bytes;
  const uint64_t ib = (uint64_t)rf->h.H * rf->h.W * rf->h.C;
  bool ok;
  if (kind == CLIP) {
    std::memcpy(&rf->F, rf->h.reserved, 4);
    ok = std::memcmp(rf->h.magic, CLIP_MAGIC, 8) == 0 && rf->F >= 1 && rf->h.C >= 1 && rf->h.C <= 4 &&
         rf->h.label_bytes == 4 && rf->h.record_bytes == (uint64_t)rf->F * ib + 4;
  } else if (kind == SEG) {
    std::memcpy(&rf->K, rf->h.reserved, 4);
    std::memcpy(&rf->kind, rf->h.reserved + 4, 4);
    const uint64_t mb = (uint64_t)rf->h.H * rf->h.W * rf->K;
    ok = std::memcmp(rf->h.magic, SEG_MAGIC, 8) == 0 && rf->K >= 1 && rf->K <= 4 && rf->kind <= 1 &&
         (rf->kind == 0 || rf->K == 1) && rf->h.C >= 1 && rf->h.C <= 4 && rf->h.label_bytes == mb &&
         rf->h.record_bytes == ib + mb;
  } else {
    ok = std::memcmp(rf->h.magic, MAGIC, 8) == 0 && rf->h.label_bytes == 4 && rf->h.record_bytes == ib + 4;
  }
  if (!ok || need > rf->size || rf->h.count == 0) {
    munmap(m, rf->size);
    close(rf->fd);
    delete rf;
    return nullptr;
  }
  madvise(m, rf->size, MADV_RANDOM);
  return rf;
}

Loader* create_loader(void* file, Kind kind, int batch, int out_h, int out_w, int train, double smin, double smax,
                      double rmin, double rmax, uint64_t seed, int rank, int world, int shuffle, int drop_last,
                      int threads, int chunk, int clip_len = 0, int frame_stride = 1, int max_tokens = 0) {
  if (!file || batch <= 0 || world <= 0 || rank < 0 || rank >= world || threads <= 0) return nullptr;
  if (((const RecordFile*)file)->what() != kind) return nullptr;   // another kind of file
  if (kind == CLIP) {   // the clip's span (T-1)*s + 1 has to fit into the record's F frames
    const int64_t F = ((const RecordFile*)file)->F;
    if (clip_len <= 0 || frame_stride <= 0 || (int64_t)(clip_len - 1) * frame_stride + 1 > F) return nullptr;
  }
  auto* L = new Loader();
  L->rf = (const RecordFile*)file;
  L->seg = kind == SEG;
  L->clip = kind == CLIP;
  L->clip_len = clip_len; L->frame_stride = frame_stride;
  L->text = kind == TEXT; L->max_tokens = max_tokens;
  L->batch = batch; L->out_h = out_h; L->out_w = out_w; L->train = train;
  L->smin = smin; L->smax = smax; L->rmin = rmin; L->rmax = rmax;
  L->seed = seed; L->rank = rank; L->world = world; L->shuffle = shuffle; L->drop_last = drop_last;
  L->chunk = chunk > 0 ? chunk : 16;
  for (int i = 0; i < threads; ++i) L->workers.emplace_back([L] { L->worker(); });
  return L;
}

int set_slot(Loader* L, int i, uint8_t* img, int64_t* lab, uint8_t* mask, int32_t* par) {
  std::lock_guard<std::mutex> lk(L->mu);
  if (L->started || i < 0) return -1;
  if ((int)L->slots.size() <= i) L->slots.resize((size_t)i + 1);
  L->slots[(size_t)i].img = img;
  L->slots[(size_t)i].lab = lab;
  L->slots[(size_t)i].mask = mask;
  L->slots[(size_t)i].par = par;
  return 0;
}

}  // namespace

MLR_EXPORT void* mlr_open(const char* path) { return open_file(path, LABELS); }

// an image + mask file; closed with mlr_close
MLR_EXPORT void* mlr_seg_open(const char* path) { return open_file(path, SEG); }

// a clip file; closed with mlr_close
MLR_EXPORT void* mlr_clip_open(const char* path) { return open_file(path, CLIP); }

// shape[0..4] = count, H, W, C, F
MLR_EXPORT void mlr_clip_shape(void* h, uint64_t* shape) {
  const auto* rf = (const RecordFile*)h;
  shape[0] = rf->h.count; shape[1] = rf->h.H; shape[2] = rf->h.W; shape[3] = rf->h.C;
  shape[4] = rf->F;
}

// shape[0..5] = count, H, W, C, K, kind
MLR_EXPORT void mlr_seg_shape(void* h, uint64_t* shape) {
  const auto* rf = (const RecordFile*)h;
  shape[0] = rf->h.count; shape[1] = rf->h.H; shape[2] = rf->h.W; shape[3] = rf->h.C;
  shape[4] = rf->K; shape[5] = rf->kind;
}

// shape[0..3] = count, H, W, C
MLR_EXPORT void mlr_shape(void* h, uint64_t* shape) {
  const auto* rf = (const RecordFile*)h;
  shape[0] = rf->h.count; shape[1] = rf->h.H; shape[2] = rf->h.W; shape[3] = rf->h.C;
}

MLR_EXPORT void mlr_close(void* h) {
  auto* rf = (RecordFile*)h;
  if (!rf) return;
  munmap((void*)rf->map, rf->size);
  close(rf->fd);
  delete rf;
}

// train != 0: RandomResizedCrop(scale [smin, smax], ratio [rmin, rmax]) + flip; else centre crop
MLR_EXPORT void* mlr_loader_create(void* file, int batch, int out_h, int out_w, int train, double smin, double smax,
                                   double rmin, double rmax, uint64_t seed, int rank, int world, int shuffle,
                                   int drop_last, int threads, int chunk) {
  return create_loader(file, LABELS, batch, out_h, out_w, train, smin, smax, rmin, rmax, seed, rank, world, shuffle,
                       drop_last, threads, chunk);
}

// register ring slot `i` (call for every slot before the first epoch)
MLR_EXPORT int mlr_loader_set_slot(void* h, int i, uint8_t* img, int64_t* lab, int32_t* par) {
  return set_slot((Loader*)h, i, img, lab, nullptr, par);
}

// the loader of an mlr_seg_open file: train != 0 draws the box as above plus hflip, vflip and
// transpose coins; start_epoch / next / release / destroy are the mlr_loader_* ones
MLR_EXPORT void* mlr_seg_loader_create(void* file, int batch, int out_h, int out_w, int train, double smin,
                                       double smax, double rmin, double rmax, uint64_t seed, int rank, int world,
                                       int shuffle, int drop_last, int threads, int chunk) {
  return create_loader(file, SEG, batch, out_h, out_w, train, smin, smax, rmin, rmax, seed, rank, world, shuffle,
                       drop_last, threads, chunk);
}

// slot `i`: image batch*H*W*C bytes, mask batch*H*W*K bytes, int32 par[batch][8]
MLR_EXPORT int mlr_seg_loader_set_slot(void* h, int i, uint8_t* img, uint8_t* mask, int32_t* par) {
  auto* L = (Loader*)h;
  if (!L->seg) return -1;
  return set_slot(L, i, img, nullptr, mask, par);
}

// the loader of an mlr_clip_open file: clips of `clip_len` frames `frame_stride` apart, one
// box and flip per clip (the mlr_loader_create draws) and then the first frame t0; null if
// (clip_len-1)*frame_stride + 1 exceeds the file's frames per record; start_epoch / next /
// release / destroy are the mlr_loader_* ones
MLR_EXPORT void* mlr_clip_loader_create(void* file, int batch, int out_h, int out_w, int clip_len, int frame_stride,
                                        int train, double smin, double smax, double rmin, double rmax,
                                        uint64_t seed, int rank, int world, int shuffle, int drop_last,
                                        int threads, int chunk) {
  return create_loader(file, CLIP, batch, out_h, out_w, train, smin, smax, rmin, rmax, seed, rank, world, shuffle,
                       drop_last, threads, chunk, clip_len, frame_stride);
}

// slot `i`: image batch*clip_len*H*W*C bytes, int64 labels[batch], int32 par[batch][8]
MLR_EXPORT int mlr_clip_loader_set_slot(void* h, int i, uint8_t* img, int64_t* lab, int32_t* par) {
  auto* L = (Loader*)h;
  if (!L->clip) return -1;
  return set_slot(L, i, img, lab, nullptr, par);
}

// a token record file; closed with mlr_close
MLR_EXPORT void* mlr_text_open(const char* path) { return open_file(path, TEXT); }

// shape[0..4] = count, longest record in tokens, vocab_size, token_bytes, total_tokens
MLR_EXPORT void mlr_text_shape(void* h, uint64_t* shape) {
  const auto* rf = (const RecordFile*)h;
  shape[0] = rf->h.count; shape[1] = rf->h.H; shape[2] = rf->h.W; shape[3] = rf->h.C;
  shape[4] = rf->total_tokens;
}

// the loader of an mlr_text_open file: batches of whole sequences, at most max_seqs of them
// (1..1024) and max_tokens tokens; null when the file's longest record is over max_len (the
// packer truncates, the loader does not) or max_len is over max_tokens; start_epoch / next /
// release / destroy are the mlr_loader_* ones
MLR_EXPORT void* mlr_text_loader_create(void* file, int max_tokens, int max_seqs, int max_len, int train,
                                        uint64_t seed, int rank, int world, int shuffle, int threads, int chunk) {
  if (!file || ((const RecordFile*)file)->what() != TEXT) return nullptr;
  if (max_seqs < 1 || max_seqs > 1024 || max_len < 1 || max_len > max_tokens ||
      ((const RecordFile*)file)->h.H > (uint32_t)max_len)
    return nullptr;
  Loader* L = create_loader(file, TEXT, max_seqs, 0, 0, train, 0, 0, 0, 0, seed, rank, world, shuffle, 0, threads,
                            chunk, 0, 1, max_tokens);
  return L;
}

// slot `i`: one int32 buffer of ((2 + 3*max_seqs + max_tokens + 1) & ~1) + 2*max_seqs ints,
// 8-byte aligned (layout: the file comment)
MLR_EXPORT int mlr_text_loader_set_slot(void* h, int i, int32_t* buf) {
  auto* L = (Loader*)h;
  if (!L->text) return -1;
  std::lock_guard<std::mutex> lk(L->mu);
  if (L->started || i < 0) return -1;
  if ((int)L->slots.size() <= i) L->slots.resize((size_t)i + 1);
  L->slots[(size_t)i].txt = buf;
  return 0;
}

// (re)start at `epoch`; returns the number of batches this rank yields in it
MLR_EXPORT int64_t mlr_loader_start_epoch(void* h, uint64_t epoch) {
  auto* L = (Loader*)h;
  {
    std::lock_guard<std::mutex> lk(L->mu);
    if (L->slots.empty()) return -1;
    for (auto& s : L->slots)
      if (L->text ? !s.txt : (!s.img || !(L->seg ? (void*)s.mask : (void*)s.lab) || !s.par)) return -1;
  }
  L->start_epoch(epoch);
  return L->nbatches;
}

MLR_EXPORT int mlr_loader_next(void* h, int64_t* batch_index) { return ((Loader*)h)->next(batch_index); }
MLR_EXPORT void mlr_loader_release(void* h, int slot) { ((Loader*)h)->release(slot); }
MLR_EXPORT void mlr_loader_destroy(void* h) { delete (Loader*)h; }
