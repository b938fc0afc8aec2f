// What the register-held end bins of census_partial (csrc/softmax_census.hpp) buy: the library's form and the form that
// sends every histogram entry through an LDS atomic, alternated on the same rotating inputs (more than 256 MB together, so no
// launch finds its input in the caches), timed per launch by device events.  Two kinds of logits at 1024 x 1024 x 2: "spread"
// (normal x 3: every bin is hit, lanes of a wave rarely share a word) and "confident" (one class leads by about 10, class 0
// on nine pixels of ten: nearly every entry in bin 0 or 255, where 64 lanes share one word).  The partial rows of the
// forms are compared byte for byte.  Not part of the library.
//   tools/_bin/census_plain [reps]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "softmax_census.hpp"

using namespace nbc::census;

#define CHECK(x)                                                                     \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) {                                                          \
      std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                   \
      return 1;                                                                      \
    }                                                                                \
  } while (0)

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static double uniform() {                            // xorshift64*, (0, 1)
  g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
  return ((g_state * 0x2545F4914F6CDD1Dull >> 11) + 0.5) / 9007199254740992.0;
}
static float normal() { return (float)(std::sqrt(-2.0 * std::log(uniform())) * std::cos(6.283185307179586 * uniform())); }

constexpr int kForms = 2;
static const char* const kFormNames[kForms] = {"end bins in registers (the library's)", "every entry an LDS atomic"};

static void launch(int form, const float* lg, const unsigned char* tg, unsigned char* plane, long long P, int T, int N, u32* pc, u32* ps,
                   u64* pb) {
  if (form == 0)
    hipLaunchKernelGGL(census_partial<true>, dim3(T, N), dim3(kThreads), 0, nullptr, lg, tg, plane, P, T, pc, ps, pb);
  else
    hipLaunchKernelGGL(census_partial<false>, dim3(T, N), dim3(kThreads), 0, nullptr, lg, tg, plane, P, T, pc, ps, pb);
}

int main(int argc, char** argv) {
  const int reps = argc > 1 ? std::atoi(argv[1]) : 100, warm = 10;
  const int N = 2, H = 1024, W = 1024;
  const long long P = (long long)H * W;
  const int T = (int)((P + kTile - 1) / kTile);
  const size_t in_bytes = (size_t)N * P * 13, count = (320u << 20) / in_bytes + 1;
  const size_t cnt_bytes = 2 * (size_t)kCounts * N * T, sum_bytes = 4 * (size_t)kSums * N * T, br_bytes = 8 * (size_t)kBrier * N * T;
  std::vector<float> host((size_t)N * 3 * P);
  std::vector<unsigned char> grey((size_t)N * P);
  u32 *pc[kForms], *ps[kForms];
  u64* pb[kForms];
  unsigned char* plane;
  for (int v = 0; v < kForms; ++v) {
    CHECK(hipMalloc(&pc[v], cnt_bytes)); CHECK(hipMalloc(&ps[v], sum_bytes)); CHECK(hipMalloc(&pb[v], br_bytes));
  }
  CHECK(hipMalloc(&plane, (size_t)N * P));
  std::vector<float*> lg(count);
  std::vector<unsigned char*> tg(count);
  for (size_t i = 0; i < count; ++i) { CHECK(hipMalloc(&lg[i], host.size() * 4)); CHECK(hipMalloc(&tg[i], grey.size())); }
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  for (int kind = 0; kind < 2; ++kind) {
    for (int n = 0; n < N; ++n)                         // one batch per kind, in `count` buffers: the addresses defeat the caches
      for (long long p = 0; p < P; ++p) {
        const double u = uniform();
        const int lead = u < 0.9 ? 0 : u < 0.95 ? 1 : 2;
        for (int c = 0; c < 3; ++c)
          host[((size_t)n * 3 + c) * P + p] = kind == 0 ? 3.f * normal() : normal() + (c == lead ? 10.f : 0.f);
        grey[(size_t)n * P + p] = (unsigned char)(uniform() * 256.0);
      }
    for (size_t i = 0; i < count; ++i) {
      CHECK(hipMemcpy(lg[i], host.data(), host.size() * 4, hipMemcpyHostToDevice));
      CHECK(hipMemcpy(tg[i], grey.data(), grey.size(), hipMemcpyHostToDevice));
    }
    std::vector<float> us[kForms];
    for (int r = 0; r < warm + reps; ++r)
      for (int v = 0; v < kForms; ++v) {               // the forms alternated on rotating inputs
        const size_t i = (size_t)(kForms * r + v) % count;
        CHECK(hipEventRecord(e0, nullptr));
        launch(v, lg[i], tg[i], plane, P, T, N, pc[v], ps[v], pb[v]);
        CHECK(hipEventRecord(e1, nullptr));
        CHECK(hipEventSynchronize(e1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= warm) us[v].push_back(ms * 1e3f);
      }
    // the same input through every form: the partial rows must not differ in a byte
    for (int v = 0; v < kForms; ++v) launch(v, lg[0], tg[0], plane, P, T, N, pc[v], ps[v], pb[v]);
    CHECK(hipDeviceSynchronize());
    std::vector<unsigned char> a(cnt_bytes + sum_bytes + br_bytes), b(a.size());
    bool same = true;
    for (int v = 0; v < kForms; ++v) {
      std::vector<unsigned char>& dst = v == 0 ? a : b;
      CHECK(hipMemcpy(dst.data(), pc[v], cnt_bytes, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(dst.data() + cnt_bytes, ps[v], sum_bytes, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(dst.data() + cnt_bytes + sum_bytes, pb[v], br_bytes, hipMemcpyDeviceToHost));
      if (v > 0) same = same && std::memcmp(a.data(), b.data(), a.size()) == 0;
    }
    for (int v = 0; v < kForms; ++v) {
      std::sort(us[v].begin(), us[v].end());
      const size_t m = us[v].size();
      std::printf("%s logits, 1024x1024x2, census_partial, %s: median %.2f us (p10 %.2f, p90 %.2f, %zu launches, event-timed)\n",
                  kind == 0 ? "spread" : "confident", kFormNames[v],
                  us[v][m / 2], us[v][m / 10], us[v][m * 9 / 10], m);
    }
    std::printf("%s logits: partial rows of the two forms %s\n", kind == 0 ? "spread" : "confident", same ? "identical" : "DIFFER");
    if (!same) return 2;
  }
  return 0;
}
