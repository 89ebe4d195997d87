// Self-test of the clip record loader (records.cpp, mlr_clip_*), built with ThreadSanitizer
// and with AddressSanitizer + UBSan by
// mlcomp_amd.build.build_runtime_selftest(main='records_clip_selftest.cpp').  It writes a
// clip file whose frames carry (record, frame) in their bytes and drives the C API from one
// consumer thread the way the python ClipRecordLoader does: several epochs, world sizes 1
// and 3, thread counts 1 and 5, epochs restarted half way, a loader destroyed while slots
// are in use.  Checks: the three readers refuse each other's files, a span longer than the
// record is refused, every epoch of a rank yields each of its samples once, the sharded
// ranks partition the file, the frames of a slot row are exactly t0 + k*stride of one
// record with its label, the boxes lie inside the image, t0 stays in [0, F - span] and
// reaches both ends, evaluation gives the centre crop of the centre frames, and runs with
// different thread counts give the same stream.  Exit status 0 = pass.
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
void mlr_close(void*);
void mlr_clip_shape(void*, uint64_t*);
void* mlr_loader_create(void*, int, int, int, int, double, double, double, double, uint64_t, int, int, int, int,
                        int, int);
void* mlr_seg_loader_create(void*, int, int, int, int, double, double, double, double, uint64_t, int, int, int,
                            int, int, int);
void* mlr_clip_loader_create(void*, int, int, int, int, int, int, double, double, double, double, uint64_t, int,
                             int, int, int, int, int);
int mlr_clip_loader_set_slot(void*, int, uint8_t*, int64_t*, int32_t*);
int mlr_seg_loader_set_slot(void*, int, uint8_t*, uint8_t*, int32_t*);
int64_t mlr_loader_start_epoch(void*, uint64_t);
int mlr_loader_next(void*, int64_t*);
void mlr_loader_release(void*, int);
void mlr_loader_destroy(void*);
}

namespace {

constexpr int H = 12, W = 10, C = 3, F = 7, T = 3, S = 2, N = 240;   // span 5: t0 in 0..2
constexpr size_t IB = (size_t)H * W * C;

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
  uint32_t a, b;   // clip files: a = F; mask files: a = K, b = kind
  uint8_t res[16];
};
static_assert(sizeof(Hdr) == 64, "header layout");

// frame t of record i: bytes (i + 3*t + 5*j) & 255 with the id in the first two and t in
// the third; label 1000 + i
void write_clip_file(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "wb");
  CHECK(f);
  Hdr hdr{};
  std::memcpy(hdr.magic, "MLVID001", 8);
  hdr.h = H; hdr.w = W; hdr.c = C; hdr.lb = 4; hdr.count = N; hdr.rb = F * IB + 4; hdr.a = F;
  std::fwrite(&hdr, sizeof(hdr), 1, f);
  std::vector<uint8_t> img(IB);
  for (int i = 0; i < N; ++i) {
    for (int t = 0; t < F; ++t) {
      for (size_t j = 0; j < IB; ++j) img[j] = (uint8_t)(i + 3 * t + 5 * j);
      img[0] = (uint8_t)(i & 255); img[1] = (uint8_t)(i >> 8); img[2] = (uint8_t)t;
      std::fwrite(img.data(), 1, IB, f);
    }
    const int32_t lab = 1000 + i;
    std::fwrite(&lab, 4, 1, f);
  }
  std::fclose(f);
}

// a label file (mask = false) or an image + mask file of the same image shape
void write_other_file(const std::string& path, bool mask) {
  FILE* f = std::fopen(path.c_str(), "wb");
  CHECK(f);
  Hdr hdr{};
  std::memcpy(hdr.magic, mask ? "MLSEG001" : "MLREC001", 8);
  const size_t tail = mask ? (size_t)H * W : 4;
  hdr.h = H; hdr.w = W; hdr.c = C; hdr.lb = (uint32_t)tail; hdr.count = 4; hdr.rb = IB + tail;
  if (mask) hdr.a = 1;
  std::fwrite(&hdr, sizeof(hdr), 1, f);
  std::vector<uint8_t> rec(IB + tail, 7);
  for (int i = 0; i < 4; ++i) std::fwrite(rec.data(), 1, rec.size(), f);
  std::fclose(f);
}

struct Ring {
  std::vector<std::vector<uint8_t>> img;
  std::vector<std::vector<int64_t>> lab;
  std::vector<std::vector<int32_t>> par;
  Ring(void* L, int depth, int batch)
      : img(depth, std::vector<uint8_t>(batch * T * IB)), lab(depth, std::vector<int64_t>(batch)),
        par(depth, std::vector<int32_t>((size_t)batch * 8)) {
    for (int i = 0; i < depth; ++i)
      CHECK(mlr_clip_loader_set_slot(L, i, img[i].data(), lab[i].data(), par[i].data()) == 0);
  }
};

// row i of slot s: the record id, after checking that frames, label and params fit together
int check_row(const Ring& r, int s, int i, int train) {
  const int32_t* p = &r.par[s][(size_t)i * 8];
  CHECK(p[2] > 0 && p[3] > 0 && p[0] >= 0 && p[1] >= 0 && p[0] + p[2] <= H && p[1] + p[3] <= W);
  CHECK(p[4] == 0 || p[4] == 1);
  CHECK(p[5] >= 0 && p[5] <= F - ((T - 1) * S + 1) && p[6] == S && p[7] == 0);
  if (!train) CHECK(p[0] == 2 && p[1] == 1 && p[2] == 8 && p[3] == 8 && !p[4] && p[5] == 1);
  const uint8_t* clip = &r.img[s][(size_t)i * T * IB];
  const int id = clip[0] | (clip[1] << 8);
  CHECK(id >= 0 && id < N);
  for (int k = 0; k < T; ++k) {   // exactly the frames t0 + k*stride of that record
    const uint8_t* im = clip + k * IB;
    const int t = p[5] + k * S;
    CHECK((im[0] | (im[1] << 8)) == id && im[2] == t);
    CHECK(im[3] == (uint8_t)(id + 3 * t + 15) && im[IB - 1] == (uint8_t)(id + 3 * t + 5 * (IB - 1)));
  }
  CHECK(r.lab[s][i] == 1000 + id);
  return id;
}

// one rank's stream for `epochs` epochs: (id, box, flip and t0) per sample; abandon_at >= 0
// restarts the next epoch after that many batches of each
std::vector<std::vector<int>> run(void* file, int batch, int world, int rank, int threads, int epochs,
                                  int abandon_at, int slow_us, int train = 1) {
  void* L = mlr_clip_loader_create(file, batch, 8, 8, T, S, train, 0.5, 1.0, 0.75, 1.333, 4321, rank, world, train,
                                   0, threads, 5);
  CHECK(L);
  Ring ring(L, 3, batch);
  std::vector<std::vector<int>> out;
  for (int e = 0; e < epochs; ++e) {
    const int64_t nb = mlr_loader_start_epoch(L, (uint64_t)e);
    CHECK(nb == (N / world + batch - 1) / batch);
    std::vector<int> seen;
    for (int64_t b = 0; b < nb; ++b) {
      if (abandon_at >= 0 && b == abandon_at) break;
      int64_t bi = -1;
      const int s = mlr_loader_next(L, &bi);
      CHECK(s >= 0 && bi == b);
      for (int i = 0; i < batch; ++i) {
        seen.push_back(check_row(ring, s, i, train));
        const int32_t* p = &ring.par[s][(size_t)i * 8];
        seen.push_back(((p[0] * 100 + p[1]) * 100 + p[2]) * 100 + p[3]);
        seen.push_back(p[4] * 10 + p[5]);
      }
      if (slow_us) std::this_thread::sleep_for(std::chrono::microseconds(slow_us));
      mlr_loader_release(L, s);
    }
    out.push_back(seen);
  }
  mlr_loader_destroy(L);
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  const std::string path = dir + "/clip_selftest.mlrec", lpath = dir + "/clip_selftest_labels.mlrec",
                    mpath = dir + "/clip_selftest_masks.mlrec";
  write_clip_file(path);
  write_other_file(lpath, false);
  write_other_file(mpath, true);
  // each of the three readers refuses the other two kinds of file
  CHECK(mlr_open(path.c_str()) == nullptr && mlr_seg_open(path.c_str()) == nullptr);
  CHECK(mlr_clip_open(lpath.c_str()) == nullptr && mlr_clip_open(mpath.c_str()) == nullptr);
  void* lf = mlr_open(lpath.c_str());
  void* mf = mlr_seg_open(mpath.c_str());
  CHECK(lf && mf);
  CHECK(mlr_clip_loader_create(lf, 4, 8, 8, 1, 1, 1, 0.5, 1.0, 0.75, 1.333, 1, 0, 1, 1, 0, 1, 4) == nullptr);
  CHECK(mlr_clip_loader_create(mf, 4, 8, 8, 1, 1, 1, 0.5, 1.0, 0.75, 1.333, 1, 0, 1, 1, 0, 1, 4) == nullptr);
  mlr_close(lf);
  mlr_close(mf);
  void* f = mlr_clip_open(path.c_str());
  CHECK(f);
  CHECK(mlr_loader_create(f, 4, 8, 8, 1, 0.5, 1.0, 0.75, 1.333, 1, 0, 1, 1, 0, 1, 4) == nullptr);
  CHECK(mlr_seg_loader_create(f, 4, 8, 8, 1, 0.5, 1.0, 0.75, 1.333, 1, 0, 1, 1, 0, 1, 4) == nullptr);
  uint64_t shp[5];
  mlr_clip_shape(f, shp);
  CHECK(shp[0] == N && shp[1] == H && shp[2] == W && shp[3] == C && shp[4] == F);
  // a span past the record's frames, or a clip without frames, is refused; the longest fits
  CHECK(mlr_clip_loader_create(f, 4, 8, 8, 4, 3, 1, 0.5, 1.0, 0.75, 1.333, 1, 0, 1, 1, 0, 1, 4) == nullptr);
  CHECK(mlr_clip_loader_create(f, 4, 8, 8, 8, 1, 1, 0.5, 1.0, 0.75, 1.333, 1, 0, 1, 1, 0, 1, 4) == nullptr);
  CHECK(mlr_clip_loader_create(f, 4, 8, 8, 0, 1, 1, 0.5, 1.0, 0.75, 1.333, 1, 0, 1, 1, 0, 1, 4) == nullptr);
  CHECK(mlr_clip_loader_create(f, 4, 8, 8, 2, 0, 1, 0.5, 1.0, 0.75, 1.333, 1, 0, 1, 1, 0, 1, 4) == nullptr);
  void* whole = mlr_clip_loader_create(f, 4, 8, 8, 7, 1, 1, 0.5, 1.0, 0.75, 1.333, 1, 0, 1, 1, 0, 1, 4);
  CHECK(whole);
  mlr_loader_destroy(whole);
  // determinism across thread counts and consumer speed
  const auto ref = run(f, 8, 1, 0, 1, 3, -1, 0);
  CHECK(run(f, 8, 1, 0, 5, 3, -1, 200) == ref);
  // each epoch is a permutation, epochs differ, t0 reaches both ends and the flip both sides
  std::set<int> t0s, flips;
  for (const auto& ep : ref) {
    std::set<int> ids;
    for (size_t i = 0; i < ep.size(); i += 3) {
      ids.insert(ep[i]);
      t0s.insert(ep[i + 2] % 10);
      flips.insert(ep[i + 2] / 10);
    }
    CHECK((int)ids.size() == N);
  }
  CHECK(ref[0] != ref[1]);
  CHECK(t0s == (std::set<int>{0, 1, 2}) && flips.size() == 2);
  // evaluation: file order, centre crop, centre frames (checked per row)
  const auto ev = run(f, 8, 1, 0, 5, 1, -1, 0, 0);
  for (int i = 0; i < N; ++i) CHECK(ev[0][(size_t)3 * i] == i);
  // sharding: 3 ranks partition every epoch, for both thread counts
  for (int th : {1, 5}) {
    std::vector<std::vector<std::vector<int>>> s;
    for (int r = 0; r < 3; ++r) s.push_back(run(f, 10, 3, r, th, 2, -1, 0));
    for (size_t e = 0; e < 2; ++e) {
      std::set<int> all;
      size_t total = 0;
      for (int r = 0; r < 3; ++r) {
        for (size_t i = 0; i < s[r][e].size(); i += 3) all.insert(s[r][e][i]);
        total += s[r][e].size() / 3;
      }
      CHECK((int)all.size() == N && (int)total == N);
    }
  }
  // start_epoch half way through an epoch restarts cleanly
  for (int th : {1, 5}) {
    const auto a = run(f, 8, 1, 0, th, 4, 2, 0);
    for (size_t e = 0; e < a.size(); ++e) {
      CHECK(a[e].size() == 3 * 2 * 8);
      if (e < ref.size()) CHECK(std::equal(a[e].begin(), a[e].end(), ref[e].begin()));
    }
  }
  // destroy while the consumer still holds slots and the workers are filling the rest
  for (int th : {1, 5}) {
    void* L = mlr_clip_loader_create(f, 8, 8, 8, T, S, 1, 0.5, 1.0, 0.75, 1.333, 9, 0, 1, 1, 0, th, 5);
    CHECK(L);
    {
      Ring ring(L, 3, 8);
      CHECK(mlr_loader_start_epoch(L, 0) == N / 8);
      int64_t bi = -1;
      CHECK(mlr_loader_next(L, &bi) == 0 && bi == 0);
      CHECK(mlr_loader_next(L, &bi) == 1 && bi == 1);
      mlr_loader_destroy(L);   // joins the workers before the ring's buffers go away
    }
  }
  // a loader without its slots does not start, and it takes no mask slot
  void* L = mlr_clip_loader_create(f, 8, 8, 8, T, S, 1, 0.5, 1.0, 0.75, 1.333, 9, 0, 1, 1, 0, 2, 5);
  CHECK(L && mlr_loader_start_epoch(L, 0) == -1);
  uint8_t dummy[8];
  int32_t dpar[8];
  CHECK(mlr_seg_loader_set_slot(L, 0, dummy, dummy, dpar) == -1);
  mlr_loader_destroy(L);
  mlr_close(f);
  std::remove(path.c_str());
  std::remove(lpath.c_str());
  std::remove(mpath.c_str());
  std::printf("records clip selftest ok\n");
  return 0;
}
