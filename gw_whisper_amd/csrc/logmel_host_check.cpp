// Stand-alone driver of the host front end (logmel_host.cpp) for `make host-sanitize`: built with the host compiler under
// -fsanitize=address,undefined and run on the CPU, outside pytest.  It runs the configurations of
// tests/test_frontend_config_host.py -- ragged and over-long inputs included -- and every refusal, and checks what needs
// no reference: finite values, the constant of the dead frames, and the published configuration bit for bit against
// gww_logmel_host_nmel_f32; and gww_logmel_windows_plan over the configurations and refusals of
// tests/test_logmel_windows_host.py against a brute-force count.  Exit status 0 when all of it holds.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/gww.h"

namespace gww {
static char g_msg[512];
int fail(int code, const char* fmt, ...) {   // the library's is in elementwise.hip
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_msg, sizeof g_msg, fmt, ap);
  va_end(ap);
  return code;
}
}  // namespace gww

static int g_bad = 0;
#define CHECK(cond, ...)           \
  do {                             \
    if (!(cond)) {                 \
      fprintf(stderr, "FAILED: "); \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");       \
      ++g_bad;                     \
    }                              \
  } while (0)

static std::vector<float> noise(size_t n, unsigned seed) {
  std::vector<float> v(n);
  unsigned long long s = 0x9E3779B97F4A7C15ull * (seed + 1);
  for (size_t i = 0; i < n; ++i) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    v[i] = (float)((double)(s >> 11) / 9007199254740992.0 - 0.5);
  }
  return v;
}

static void run(const gww_frontend_cfg& c, int n_in, int n_seg) {
  const int frames = c.n_samples / c.hop_length;
  const int n_eff = n_in < c.n_samples ? n_in : c.n_samples;
  std::vector<float> w = noise((size_t)n_seg * (n_in > 0 ? n_in : 1), (unsigned)(c.n_fft + n_in));
  std::vector<float> out((size_t)n_seg * c.n_mels * frames, NAN);
  const int rc = gww_logmel_host_cfg_f32(&c, w.data(), n_seg, n_in, n_in > 0 ? n_in : 1, out.data());
  CHECK(rc == GWW_OK, "n_fft %d hop %d n_samples %d, input %d: rc %d (%s)", c.n_fft, c.hop_length, c.n_samples, n_in, rc,
        gww::g_msg);
  if (rc != GWW_OK) return;
  long live = ((long)n_eff + c.n_fft / 2 + c.hop_length - 1) / c.hop_length;
  if (n_eff >= c.n_samples - c.n_fft || live > frames) live = frames;
  for (int s = 0; s < n_seg; ++s)
    for (int m = 0; m < c.n_mels; ++m) {
      const float* row = out.data() + ((size_t)s * c.n_mels + m) * frames;
      for (int t = 0; t < frames; ++t) CHECK(isfinite(row[t]), "non-finite value at [%d, %d, %d]", s, m, t);
      for (long t = live; t < frames; ++t)
        CHECK(memcmp(&row[t], &row[frames - 1], 4) == 0, "dead frame %ld of row %d differs (n_fft %d)", t, m, c.n_fft);
    }
  printf("ok  mels %3d rate %5d hop %3d n_fft %4d samples %6d fmax %6g  input %6d x %d: %d frames, %ld live\n", c.n_mels,
         c.sampling_rate, c.hop_length, c.n_fft, c.n_samples, (double)c.max_frequency, n_in, n_seg, frames, live);
}

static void refuse(gww_frontend_cfg c, const char* field) {
  float x[4] = {0, 0, 0, 0}, o[4];
  const int rc = gww_logmel_host_cfg_f32(&c, x, 1, 4, 4, o);
  CHECK(rc == GWW_ERR_ARG && strstr(gww::g_msg, field), "expected a refusal naming %s, got rc %d (%s)", field, rc, gww::g_msg);
  if (rc == GWW_ERR_ARG) printf("ok  refused: %s\n", gww::g_msg);
  const int rv = gww_frontend_validate_cfg(&c);   // the validator on its own: the same refusal, no data
  CHECK(rv == GWW_ERR_ARG && strstr(gww::g_msg, field), "validate: expected a refusal naming %s, got rc %d (%s)", field, rv,
        gww::g_msg);
}

// gww_logmel_windows_plan against a brute-force count: loop over windows and frames, classify each by the two
// inequalities of include/gww.h, put the centres of the interior ones into a set (a sorted vector here)
static void plan_case(int n_fft, int hop, int L, int step, int n) {
  const gww_frontend_cfg c = {80, 2048, n_fft, hop, L, 0.f, 1024.f};
  gww_windows_plan p;
  memset(&p, 0xEE, sizeof p);
  const int rc = gww_logmel_windows_plan(&c, step, n, &p);
  CHECK(rc == GWW_OK, "windows plan n_fft %d hop %d L %d step %d n %d: rc %d (%s)", n_fft, hop, L, step, n, rc, gww::g_msg);
  if (rc != GWW_OK) return;
  const int H = n_fft / 2, F = L / hop;
  long lo = 0, hi = 0;
  std::vector<long> centres;
  for (int w = 0; w < n; ++w)
    for (int t = 0; t < F; ++t) {
      if (t * hop < H) ++lo;
      else if (t * hop + H > L) ++hi;
      else centres.push_back((long)w * step + (long)t * hop);
    }
  std::sort(centres.begin(), centres.end());
  // (a step that is no multiple of the hop: the plan models no sharing at all -- the kernels share none -- although every
  // few windows line up again)
  const long distinct = step % hop ? (long)centres.size() : (long)(std::unique(centres.begin(), centres.end()) - centres.begin());
  const long shared_frames = distinct + lo + hi, per_window = (long)n * F;
  const bool shared = step % hop == 0 && shared_frames < per_window;
  CHECK(p.edge_lo == lo / n && p.edge_hi == hi / n && p.interior == F - lo / n - hi / n, "windows plan: edges %d + %d + %d, want "
        "%ld + %ld", p.edge_lo, p.interior, p.edge_hi, lo / n, hi / n);
  CHECK(p.stream_frames == distinct && p.dft_frames_shared == shared_frames && p.dft_frames_per_window == per_window,
        "windows plan n_fft %d hop %d L %d step %d n %d: %ld stream / %ld shared / %ld per window, want %ld / %ld / %ld", n_fft,
        hop, L, step, n, p.stream_frames, p.dft_frames_shared, p.dft_frames_per_window, distinct, shared_frames, per_window);
  CHECK(p.route == (shared ? GWW_WINDOWS_SHARED : GWW_WINDOWS_PER_WINDOW), "windows plan: route %d", p.route);
  const long floats = shared ? 80 * (distinct + lo + hi) : n;
  CHECK(p.workspace_bytes == (floats * 4 + 15) / 16 * 16, "windows plan: workspace %ld", p.workspace_bytes);
  printf("ok  windows n_fft %4d hop %3d L %5d step %4d n %4d: %d + %d + %d frames, %ld shared / %ld per window -> %s\n", n_fft,
         hop, L, step, n, p.edge_lo, p.interior, p.edge_hi, p.dft_frames_shared, p.dft_frames_per_window,
         p.route == GWW_WINDOWS_SHARED ? "shared" : "per window");
}

static void plan_refuse(gww_frontend_cfg c, int step, int n, const char* name) {
  gww_windows_plan p;
  const int rc = gww_logmel_windows_plan(&c, step, n, &p);
  CHECK(rc == GWW_ERR_ARG && strstr(gww::g_msg, name), "windows plan: expected a refusal naming %s, got rc %d (%s)", name, rc,
        gww::g_msg);
  if (rc == GWW_ERR_ARG) printf("ok  refused: %s\n", gww::g_msg);
}

int main() {
  // the windows of a series: tests/test_logmel_windows_host.py
  const int plans[][4] = {{16, 4, 128, 8},  {18, 6, 132, 12}, {16, 16, 256, 32}, {128, 12, 2048, 204}, {16, 4, 128, 4},
                          {16, 4, 128, 128}, {16, 4, 128, 10}, {16, 4, 128, 512}, {64, 8, 40, 8},       {64, 8, 2048, 200}};
  for (const auto& q : plans)
    for (int n : {1, 2, 7, 256}) plan_case(q[0], q[1], q[2], q[3], n);
  {
    const gww_frontend_cfg w = {80, 2048, 128, 12, 2048, 0.f, 1024.f};
    gww_windows_plan p;
    CHECK(gww_logmel_windows_plan(&w, 204, 256, &p) == GWW_OK && p.edge_lo == 6 && p.edge_hi == 4 && p.interior == 160 &&
              p.stream_frames == 17 * 255 + 160 && p.route == GWW_WINDOWS_SHARED,
          "windows plan: the workload's counts");
    plan_refuse(w, 0, 4, "step");
    plan_refuse(w, -204, 4, "step");
    plan_refuse(w, 204, 0, "n_windows");
    plan_refuse(w, 204, -3, "n_windows");
    gww_frontend_cfg b = w;
    b.n_fft = 127;
    plan_refuse(b, 204, 4, "n_fft");
    CHECK(gww_logmel_windows_plan(&w, 204, 4, nullptr) == GWW_ERR_ARG && strstr(gww::g_msg, "out"), "NULL plan accepted");
    CHECK(gww_logmel_windows_plan(nullptr, 204, 4, &p) == GWW_ERR_ARG, "NULL cfg accepted by the windows plan");
  }

  // (mels, rate, n_fft, hop, chunk samples, fmin, fmax) and the input length: tests/test_frontend_config_host.py
  const struct { gww_frontend_cfg c; int n_in; } cases[] = {
      {{80, 2048, 128, 16, 4096, 0.f, 8000.f}, 2048},
      {{80, 2048, 128, 16, 4096, 0.f, 1024.f}, 2048},
      {{80, 16000, 400, 160, 32000, 0.f, 8000.f}, 16000},
      {{80, 16000, 400, 160, 16000, 0.f, 8000.f}, 16000},
      {{128, 4000, 250, 25, 4000, 0.f, 2000.f}, 3000},
      {{80, 4096, 1024, 256, 16384, 0.f, 2048.f}, 5000},
      {{80, 2048, 64, 8, 2048, 0.f, 1024.f}, 2048},
  };
  for (const auto& k : cases) {
    CHECK(gww_frontend_validate_cfg(&k.c) == GWW_OK, "validate refused a supported configuration (%s)", gww::g_msg);
    run(k.c, k.n_in, 2);
    run(k.c, 0, 1);                        // an empty input
    run(k.c, 1, 1);
    run(k.c, k.c.n_samples + 37, 1);       // truncated at the chunk
  }
  run({80, 8000, 1018, 1018, 8144, 0.f, 4000.f}, 8144, 1);   // n_fft / 2 prime, hop = n_fft
  run({128, 16000, 16, 1, 3000, 0.f, 8000.f}, 2000, 1);      // the smallest n_fft, 3000 frames

  // the published configuration: bit for bit the fixed entry point
  for (int nm : {80, 128}) {
    const gww_frontend_cfg d = {nm, 16000, 400, 160, 480000, 0.f, 8000.f};
    std::vector<float> w = noise(2 * 16000, 7);
    std::vector<float> a((size_t)2 * nm * 3000), b(a.size());
    CHECK(gww_logmel_host_cfg_f32(&d, w.data(), 2, 16000, 16000, a.data()) == GWW_OK, "default cfg failed");
    CHECK(gww_logmel_host_nmel_f32(w.data(), 2, 16000, 16000, nm, b.data()) == GWW_OK, "default nmel failed");
    CHECK(memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0, "published configuration differs (n_mels %d)", nm);
  }

  const gww_frontend_cfg g = {80, 2048, 128, 16, 4096, 0.f, 1024.f};
  gww_frontend_cfg c;
  c = g; c.n_mels = 64; refuse(c, "n_mels");
  c = g; c.n_fft = 127; refuse(c, "n_fft");
  c = g; c.n_fft = 2048; refuse(c, "n_fft");
  c = g; c.n_fft = 8; refuse(c, "n_fft");
  c = g; c.hop_length = 0; refuse(c, "hop_length");
  c = g; c.hop_length = 129; refuse(c, "hop_length");
  c = g; c.n_samples = 64; refuse(c, "n_samples");
  c = g; c.n_samples = 16 * 3001; refuse(c, "n_frames");
  c = g; c.min_frequency = -1.f; refuse(c, "min_frequency");
  c = g; c.max_frequency = 0.f; refuse(c, "max_frequency");
  c = g; c.sampling_rate = 0; refuse(c, "sampling_rate");
  CHECK(gww_logmel_host_cfg_f32(nullptr, nullptr, 0, 0, 0, nullptr) == GWW_ERR_ARG, "NULL cfg accepted");
  CHECK(gww_frontend_validate_cfg(nullptr) == GWW_ERR_ARG, "validate accepted a NULL cfg");
  if (g_bad) {
    fprintf(stderr, "%d check(s) failed\n", g_bad);
    return 1;
  }
  printf("host front end: all checks passed\n");
  return 0;
}
