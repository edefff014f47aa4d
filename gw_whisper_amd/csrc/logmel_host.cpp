// Host (CPU) log-mel front end: the fork-safe twin of gww_logmel_f32.
//
// Replaces WhisperFeatureExtractor.__call__ where the reference calls it from forked DataLoader workers
// (Signal_vs_Noise/src/dataset.py:12,20-21 under src/train.py:224-225, num_workers 12): a worker may not touch
// the GPU, so this entry point is plain C++ -- no HIP call, no device memory, no global mutable state (the tables
// are function-local statics, built once, thread safe since C++11).  Same arithmetic as
// HF:models/whisper/feature_extraction_whisper.py:135-168: zero-pad to 480000 -> reflect-pad 200 -> 400-point
// periodic-Hann DFT, hop 160 -> |X|^2 (frames 0..2999) -> mel[n_mels,201] @ P -> log10(max(., 1e-10)) -> per-segment
// max -> max(x, max - 8) -> (x + 4) / 4, with the same exact shortcut as the device kernel: frames that only see
// zero padding are the one constant HF produces for them.  n_mels is 80 or 128 (whisper-large-v3), one table set each.
//
// The DFT is a 200-point complex mixed-radix FFT (5 x 5 x 4 x 2, decimation in time) of the even / odd samples of
// the windowed frame followed by the real-input untangling step; double precision, rounded to fp32 once per mel.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/gww.h"

namespace gww {
int fail(int code, const char* fmt, ...);   // elementwise.hip (per-thread error text)
}

namespace {

constexpr int kNfft = 400, kHalf = 200, kHop = 160, kNfreq = 201, kMaxMel = 128, kFrames = 3000, kChunk = 480000;
constexpr double kPi = 3.14159265358979323846;

struct Cpx {
  double re, im;
};

struct HostTables {
  double win[kNfft];
  Cpx w200[kHalf];        // exp(-2 pi i k / 200)
  Cpx w400[kHalf + 1];    // exp(-2 pi i k / 400), k = 0..200
  int n_mels;
  // sparse filterbank: HF's dense [201, n_mels] slaney triangles touch at most a few mels per bin
  int fb_first[kNfreq], fb_count[kNfreq];
  std::vector<float> fb_val;   // the fp32-cast weights HF multiplies with
  std::vector<int> fb_ofs;

  static double hz2mel(double f) { return f >= 1000.0 ? 15.0 + log(f / 1000.0) * (27.0 / log(6.4)) : 3.0 * f / 200.0; }
  static double mel2hz(double m) { return m >= 15.0 ? 1000.0 * exp((log(6.4) / 27.0) * (m - 15.0)) : 200.0 * m / 3.0; }

  explicit HostTables(int nm) : n_mels(nm) {
    const int kNmel = nm;
    for (int k = 0; k < kNfft; ++k) win[k] = (double)(float)(0.5 - 0.5 * cos(2.0 * kPi * k / kNfft));
    for (int k = 0; k < kHalf; ++k) w200[k] = {cos(2.0 * kPi * k / kHalf), -sin(2.0 * kPi * k / kHalf)};
    for (int k = 0; k <= kHalf; ++k) w400[k] = {cos(2.0 * kPi * k / kNfft), -sin(2.0 * kPi * k / kNfft)};
    // HF:audio_utils.py:638-731 (slaney scale + slaney norm, 0..8000 Hz)
    const double mel_min = hz2mel(0.0), mel_max = hz2mel(8000.0);
    double ff[kNmel + 2];
    for (int i = 0; i < kNmel + 2; ++i) ff[i] = mel2hz(mel_min + (mel_max - mel_min) * i / (kNmel + 1));
    fb_ofs.resize(kNfreq);
    for (int k = 0; k < kNfreq; ++k) {
      const double fk = 8000.0 * k / (kNfreq - 1);
      fb_first[k] = 0;
      fb_count[k] = 0;
      fb_ofs[k] = (int)fb_val.size();
      int last = -1;
      float row[kMaxMel];
      for (int m = 0; m < kNmel; ++m) {
        const double down = (fk - ff[m]) / (ff[m + 1] - ff[m]);
        const double up = (ff[m + 2] - fk) / (ff[m + 2] - ff[m + 1]);
        double v = down < up ? down : up;
        if (v < 0) v = 0;
        v *= 2.0 / (ff[m + 2] - ff[m]);
        row[m] = (float)v;
        if (row[m] != 0.0f) {
          if (last < 0) fb_first[k] = m;
          last = m;
        }
      }
      if (last >= 0) {
        fb_count[k] = last - fb_first[k] + 1;
        for (int m = fb_first[k]; m <= last; ++m) fb_val.push_back(row[m]);
      }
    }
  }
};

const HostTables& tables(int n_mels) {
  static const HostTables t80(80), t128(128);
  return n_mels == 128 ? t128 : t80;
}

// out[0..n) = DFT_n(in[0], in[stride], ...); n divides 200, twiddles from the 200-entry table.
void fft_rec(int n, const Cpx* in, int stride, Cpx* out, const HostTables& tb) {
  if (n == 1) {
    out[0] = in[0];
    return;
  }
  const int p = (n % 5 == 0) ? 5 : (n % 4 == 0) ? 4 : 2;
  const int m = n / p;
  for (int q = 0; q < p; ++q) fft_rec(m, in + (long)q * stride, stride * p, out + q * m, tb);
  const int tw = kHalf / n;   // w_n^j = w200[j * tw]
  for (int k = 0; k < m; ++k) {
    Cpx t[5];
    for (int q = 0; q < p; ++q) {
      const Cpx a = out[q * m + k];
      const Cpx w = tb.w200[(q * k * tw) % kHalf];
      t[q] = {a.re * w.re - a.im * w.im, a.re * w.im + a.im * w.re};
    }
    for (int r = 0; r < p; ++r) {
      double sr = t[0].re, si = t[0].im;
      for (int q = 1; q < p; ++q) {
        const Cpx w = tb.w200[((q * r) % p) * (kHalf / p)];
        sr += t[q].re * w.re - t[q].im * w.im;
        si += t[q].re * w.im + t[q].im * w.re;
      }
      out[k + r * m] = {sr, si};
    }
  }
}

// power[k] = |rfft(frame)[k]|^2, k = 0..200, of one windowed 400-sample frame
void frame_power(const double* frame, double* power, const HostTables& tb) {
  Cpx z[kHalf], Z[kHalf];
  for (int n = 0; n < kHalf; ++n) z[n] = {frame[2 * n], frame[2 * n + 1]};
  fft_rec(kHalf, z, 1, Z, tb);
  for (int k = 0; k <= kHalf; ++k) {
    const Cpx a = Z[k % kHalf];
    const Cpx b = {Z[(kHalf - k) % kHalf].re, -Z[(kHalf - k) % kHalf].im};
    const Cpx e = {0.5 * (a.re + b.re), 0.5 * (a.im + b.im)};       // FFT of the even samples
    const Cpx o = {0.5 * (a.im - b.im), -0.5 * (a.re - b.re)};      // FFT of the odd samples: (a - b) / (2i)
    const Cpx w = tb.w400[k];
    const double re = e.re + o.re * w.re - o.im * w.im;
    const double im = e.im + o.re * w.im + o.im * w.re;
    power[k] = re * re + im * im;
  }
}

}  // namespace

extern "C" int gww_logmel_host_nmel_f32(const float* wave, int n_seg, int n_samples, long wave_stride, int n_mels,
                                        float* out) {
  if (!wave || !out) return gww::fail(GWW_ERR_ARG, "gww_logmel_host_f32: NULL argument");
  if (n_seg < 0 || n_samples < 0) return gww::fail(GWW_ERR_ARG, "gww_logmel_host_f32: negative size");
  if (n_mels != 80 && n_mels != 128) return gww::fail(GWW_ERR_ARG, "gww_logmel_host_f32: n_mels=%d (80 or 128)", n_mels);
  const int n_eff = n_samples < kChunk ? n_samples : kChunk;   // HF truncates at 30 s
  if (wave_stride < n_eff)
    return gww::fail(GWW_ERR_ARG, "gww_logmel_host_f32: wave_stride %ld < n_samples %d", wave_stride, n_samples);
  const HostTables& tb = tables(n_mels);
  const int kNmel = n_mels;
  int live = kFrames;
  if (n_eff < kChunk - kNfft) {
    live = (n_eff + kNfft / 2 + kHop - 1) / kHop;
    if (live > kFrames) live = kFrames;
    if (live < 1) live = 1;
  }
  std::vector<float> raw((size_t)kNmel * live);
  for (int s = 0; s < n_seg; ++s) {
    const float* x = wave + (long)s * wave_stride;
    float* o = out + (size_t)s * kNmel * kFrames;
    // sample of the zero-padded, reflect-padded buffer at padded index j (buffer index j - 200)
    auto sample = [&](long j) -> double {
      long i = j - kNfft / 2;
      if (i < 0) i = -i;                                  // reflect (no edge repeat)
      if (i >= kChunk) i = 2L * (kChunk - 1) - i;
      return i < n_eff ? (double)x[i] : 0.0;
    };
    float seg_max = -INFINITY;
    for (int t = 0; t < live; ++t) {
      double frame[kNfft], power[kNfreq], mel[kMaxMel];
      for (int n = 0; n < kNfft; ++n) frame[n] = sample((long)t * kHop + n) * tb.win[n];
      frame_power(frame, power, tb);
      for (int m = 0; m < kNmel; ++m) mel[m] = 0.0;
      for (int k = 0; k < kNfreq; ++k) {
        const float pk = (float)power[k];                 // HF's magnitudes are fp32
        const float* v = tb.fb_val.data() + tb.fb_ofs[k];
        for (int c = 0; c < tb.fb_count[k]; ++c) mel[tb.fb_first[k] + c] += (double)v[c] * (double)pk;
      }
      for (int m = 0; m < kNmel; ++m) {
        float v = (float)mel[m];
        if (v < 1e-10f) v = 1e-10f;
        const float lg = (float)log10((double)v);
        raw[(size_t)m * live + t] = lg;
        if (lg > seg_max) seg_max = lg;
      }
    }
    if (live < kFrames && -10.0f > seg_max) seg_max = -10.0f;   // the dead frames' log10(1e-10) takes part in the max
    const float floor_v = seg_max - 8.0f;
    const float dead = ((-10.0f > floor_v ? -10.0f : floor_v) + 4.0f) / 4.0f;
    for (int m = 0; m < kNmel; ++m) {
      float* row = o + (size_t)m * kFrames;
      const float* r = raw.data() + (size_t)m * live;
      for (int t = 0; t < live; ++t) row[t] = ((r[t] > floor_v ? r[t] : floor_v) + 4.0f) / 4.0f;
      for (int t = live; t < kFrames; ++t) row[t] = dead;
    }
  }
  return GWW_OK;
}

extern "C" int gww_logmel_host_f32(const float* wave, int n_seg, int n_samples, long wave_stride, float* out) {
  return gww_logmel_host_nmel_f32(wave, n_seg, n_samples, wave_stride, 80, out);
}

// ---- any configuration (HF: WhisperFeatureExtractor(feature_size, sampling_rate, hop_length, chunk_length, n_fft)) ----
// The supported set, the frame arithmetic and the tables are defined once, here, in plain C++: the device handle
// (logmel.hip) calls the same three functions, so both twins hold one window and one filterbank.
namespace gww {

// GWW_OK, or GWW_ERR_ARG with a message that names the offending field
int frontend_validate(const gww_frontend_cfg* c, const char* who) {
  if (!c) return fail(GWW_ERR_ARG, "%s: cfg is NULL", who);
  if (c->n_mels != 80 && c->n_mels != 128) return fail(GWW_ERR_ARG, "%s: n_mels=%d (80 or 128)", who, c->n_mels);
  if (c->sampling_rate < 2) return fail(GWW_ERR_ARG, "%s: sampling_rate=%d must be at least 2", who, c->sampling_rate);
  if (c->n_fft < 16 || c->n_fft > 1024 || c->n_fft % 2)
    return fail(GWW_ERR_ARG, "%s: n_fft=%d must be even and in [16, 1024]", who, c->n_fft);
  if (c->hop_length < 1 || c->hop_length > c->n_fft)
    return fail(GWW_ERR_ARG, "%s: hop_length=%d must be in [1, n_fft=%d]", who, c->hop_length, c->n_fft);
  if (c->n_samples <= c->n_fft / 2)
    return fail(GWW_ERR_ARG, "%s: n_samples=%d must exceed n_fft / 2 = %d (the reflect pad)", who, c->n_samples, c->n_fft / 2);
  const long frames = (long)c->n_samples / c->hop_length;
  if (frames < 1 || frames > 3000)
    return fail(GWW_ERR_ARG, "%s: n_frames=%ld (n_samples / hop_length) must be in [1, 3000]", who, frames);
  if (!(c->min_frequency >= 0.0f)) return fail(GWW_ERR_ARG, "%s: min_frequency=%g must be >= 0", who, (double)c->min_frequency);
  if (!(c->max_frequency > c->min_frequency))
    return fail(GWW_ERR_ARG, "%s: max_frequency=%g must exceed min_frequency=%g", who, (double)c->max_frequency,
                (double)c->min_frequency);
  return GWW_OK;
}

// frames that can see a non-zero sample of an input of n_eff samples: frame t covers [hop t - n_fft / 2, hop t + n_fft / 2)
// of the zero-padded buffer; the reflection at its far end reaches back less than n_fft samples
int frontend_live_frames(const gww_frontend_cfg* c, int n_eff) {
  const int frames = c->n_samples / c->hop_length;
  if (n_eff >= c->n_samples - c->n_fft) return frames;
  long live = ((long)n_eff + c->n_fft / 2 + c->hop_length - 1) / c->hop_length;
  if (live > frames) live = frames;
  if (live < 1) live = 1;
  return (int)live;
}

// win / cost / sint [n_fft]: the periodic Hann and the twiddles, rounded to fp32 once; fbT [n_fft / 2 + 1][n_mels]: HF's
// mel_filter_bank(n_fft / 2 + 1, n_mels, min_frequency, max_frequency, sampling_rate, "slaney", "slaney"), rounded to fp32
void frontend_tables(const gww_frontend_cfg* c, float* win, float* cost, float* sint, float* fbT) {
  const int N = c->n_fft, nfreq = N / 2 + 1, nm = c->n_mels;
  for (int k = 0; k < N; ++k) {
    win[k] = (float)(0.5 - 0.5 * cos(2.0 * kPi * k / N));
    if (cost) cost[k] = (float)cos(2.0 * kPi * k / N);
    if (sint) sint[k] = (float)sin(2.0 * kPi * k / N);
  }
  const double mel_min = HostTables::hz2mel((double)c->min_frequency), mel_max = HostTables::hz2mel((double)c->max_frequency);
  std::vector<double> ff(nm + 2);
  for (int i = 0; i < nm + 2; ++i) ff[i] = HostTables::mel2hz(mel_min + (mel_max - mel_min) * i / (nm + 1));
  const double nyq = (double)(c->sampling_rate / 2);   // HF: linspace(0, sampling_rate // 2, n_freq)
  for (int k = 0; k < nfreq; ++k) {
    const double fk = nyq * k / (nfreq - 1);
    for (int m = 0; m < nm; ++m) {
      const double down = (fk - ff[m]) / (ff[m + 1] - ff[m]);
      const double up = (ff[m + 2] - fk) / (ff[m + 2] - ff[m + 1]);
      double v = down < up ? down : up;
      if (v < 0) v = 0;
      v *= 2.0 / (ff[m + 2] - ff[m]);
      fbT[(size_t)k * nm + m] = (float)v;
    }
  }
}

// The windows of a series (include/gww.h: gww_windows_plan): which frames of a window see its reflect padding, how many
// distinct interior frames n windows hold, and the route that follows.  No GPU call.
//   edge at the start:  t hop < n_fft / 2            <=>  t < ceil((n_fft / 2) / hop)
//   edge at the end:    t hop + n_fft / 2 > L        <=>  t > (L - n_fft / 2) / hop
// With step = s hop, interior frame t of window w is frame w s + t of one hop-spaced stream: n windows hold
// (n - 1) min(s, interior) + interior distinct ones.
int logmel_windows_plan(const gww_frontend_cfg* c, int step, int n_windows, gww_windows_plan* out, const char* who) {
  if (int rc = frontend_validate(c, who)) return rc;
  if (!out) return fail(GWW_ERR_ARG, "%s: out is NULL", who);
  if (step < 1) return fail(GWW_ERR_ARG, "%s: step=%d must be at least 1", who, step);
  if (n_windows < 1) return fail(GWW_ERR_ARG, "%s: n_windows=%d must be at least 1", who, n_windows);
  const int H = c->n_fft / 2, hop = c->hop_length, L = c->n_samples, F = L / hop;
  const long n = n_windows;
  int lo = (H + hop - 1) / hop;
  if (lo > F) lo = F;
  int hi0 = (L - H) / hop + 1;            // the first frame that reaches past the window's last sample
  if (hi0 > F) hi0 = F;
  if (hi0 < lo) hi0 = lo;                 // (a frame that is an edge at both ends counts once)
  out->edge_lo = lo;
  out->edge_hi = F - hi0;
  out->interior = hi0 - lo;
  const bool aligned_step = step % hop == 0;
  const long s = step / hop;
  out->stream_frames = aligned_step && out->interior > 0 ? (n - 1) * (s < out->interior ? s : out->interior) + out->interior
                                                         : n * out->interior;
  out->dft_frames_shared = out->stream_frames + n * (out->edge_lo + out->edge_hi);
  out->dft_frames_per_window = n * F;
  const bool shared = aligned_step && out->dft_frames_shared < out->dft_frames_per_window;
  out->route = shared ? GWW_WINDOWS_SHARED : GWW_WINDOWS_PER_WINDOW;
  // shared: raw stream [n_mels, stream_frames] + raw edges [n_windows, n_mels, edges]; per window: one maximum each
  const long floats = shared ? (long)c->n_mels * (out->stream_frames + n * (out->edge_lo + out->edge_hi)) : n;
  out->workspace_bytes = (floats * 4 + 15) / 16 * 16;
  return GWW_OK;
}

}  // namespace gww

extern "C" int gww_logmel_windows_plan(const gww_frontend_cfg* cfg, int step, int n_windows, gww_windows_plan* out) {
  return gww::logmel_windows_plan(cfg, step, n_windows, out, "gww_logmel_windows_plan");
}

namespace {

// out[0..n) = DFT_n(in[0], in[stride], ...) by decimation in time over the prime factors of n (4 before 2); n divides H,
// w[k] = exp(-2 pi i k / H); t: scratch for one butterfly (the largest prime factor of H)
void fft_any(int n, const Cpx* in, long stride, Cpx* out, const Cpx* w, int H, Cpx* t) {
  if (n == 1) {
    out[0] = in[0];
    return;
  }
  int p = n;
  if (n % 4 == 0) p = 4;
  else if (n % 2 == 0) p = 2;
  else
    for (int q = 3; q * q <= n; q += 2)
      if (n % q == 0) {
        p = q;
        break;
      }
  const int m = n / p;
  for (int q = 0; q < p; ++q) fft_any(m, in + (long)q * stride, stride * p, out + q * m, w, H, t);
  const int tw = H / n, tp = H / p;
  for (int k = 0; k < m; ++k) {
    for (int q = 0; q < p; ++q) {
      const Cpx a = out[q * m + k];
      const Cpx ww = w[(int)(((long)q * k * tw) % H)];
      t[q] = {a.re * ww.re - a.im * ww.im, a.re * ww.im + a.im * ww.re};
    }
    for (int r = 0; r < p; ++r) {
      double sr = t[0].re, si = t[0].im;
      for (int q = 1; q < p; ++q) {
        const Cpx ww = w[(int)(((long)q * r) % p) * tp];
        sr += t[q].re * ww.re - t[q].im * ww.im;
        si += t[q].re * ww.im + t[q].im * ww.re;
      }
      out[k + r * m] = {sr, si};
    }
  }
}

bool is_whisper_default(const gww_frontend_cfg* c) {
  return c->sampling_rate == 16000 && c->n_fft == kNfft && c->hop_length == kHop && c->n_samples == kChunk &&
         c->min_frequency == 0.0f && c->max_frequency == 8000.0f;
}

}  // namespace

extern "C" int gww_frontend_validate_cfg(const gww_frontend_cfg* cfg) {
  return gww::frontend_validate(cfg, "gww_frontend_validate_cfg");
}

extern "C" int gww_frontend_mel_filters_host_f32(const gww_frontend_cfg* cfg, float* out) {
  if (int rc = gww::frontend_validate(cfg, "gww_frontend_mel_filters_host_f32")) return rc;
  if (!out) return gww::fail(GWW_ERR_ARG, "gww_frontend_mel_filters_host_f32: out is NULL");
  const int N = cfg->n_fft, nfreq = N / 2 + 1, nm = cfg->n_mels;
  std::vector<float> win(N), fb((size_t)nfreq * nm);
  gww::frontend_tables(cfg, win.data(), nullptr, nullptr, fb.data());
  for (int k = 0; k < nfreq; ++k)
    for (int m = 0; m < nm; ++m) out[(size_t)m * nfreq + k] = fb[(size_t)k * nm + m];
  return GWW_OK;
}

extern "C" int gww_logmel_host_cfg_f32(const gww_frontend_cfg* cfg, const float* wave, int n_seg, int n_samples_in,
                                       long wave_stride, float* out) {
  const char* who = "gww_logmel_host_cfg_f32";
  if (int rc = gww::frontend_validate(cfg, who)) return rc;
  if (!wave || !out) return gww::fail(GWW_ERR_ARG, "%s: NULL argument", who);
  if (n_seg < 0 || n_samples_in < 0) return gww::fail(GWW_ERR_ARG, "%s: negative size", who);
  // Whisper's published configuration keeps its own 200-point FFT and tables: one result, bit for bit, by either entry
  if (is_whisper_default(cfg)) return gww_logmel_host_nmel_f32(wave, n_seg, n_samples_in, wave_stride, cfg->n_mels, out);
  const int N = cfg->n_fft, H = N / 2, nfreq = H + 1, hop = cfg->hop_length, chunk = cfg->n_samples, nm = cfg->n_mels;
  const int frames = chunk / hop;
  const int n_eff = n_samples_in < chunk ? n_samples_in : chunk;   // HF truncates at chunk_length
  if (wave_stride < n_eff) return gww::fail(GWW_ERR_ARG, "%s: wave_stride %ld < n_samples %d", who, wave_stride, n_samples_in);
  const int live = gww::frontend_live_frames(cfg, n_eff);

  std::vector<float> win32(N), fb((size_t)nfreq * nm);
  gww::frontend_tables(cfg, win32.data(), nullptr, nullptr, fb.data());
  std::vector<int> fb_first(nfreq, 0), fb_count(nfreq, 0);      // the non-zero run of mels per bin
  for (int k = 0; k < nfreq; ++k) {
    int first = -1, last = -1;
    for (int m = 0; m < nm; ++m)
      if (fb[(size_t)k * nm + m] != 0.0f) {
        if (first < 0) first = m;
        last = m;
      }
    if (first >= 0) {
      fb_first[k] = first;
      fb_count[k] = last - first + 1;
    }
  }
  std::vector<Cpx> wH(H), wN(H + 1), z(H), Z(H), scratch(H);
  for (int k = 0; k < H; ++k) wH[k] = {cos(2.0 * kPi * k / H), -sin(2.0 * kPi * k / H)};
  for (int k = 0; k <= H; ++k) wN[k] = {cos(2.0 * kPi * k / N), -sin(2.0 * kPi * k / N)};
  std::vector<double> frame(N), mel(nm);
  std::vector<float> raw((size_t)nm * live);

  for (int s = 0; s < n_seg; ++s) {
    const float* x = wave + (long)s * wave_stride;
    float* o = out + (size_t)s * nm * frames;
    auto sample = [&](long j) -> double {        // padded index j <-> buffer index j - n_fft / 2, reflected once
      long i = j - H;
      if (i < 0) i = -i;
      if (i >= chunk) i = 2L * (chunk - 1) - i;
      return i < n_eff ? (double)x[i] : 0.0;
    };
    float seg_max = -INFINITY;
    for (int t = 0; t < live; ++t) {
      for (int n = 0; n < N; ++n) frame[n] = sample((long)t * hop + n) * (double)win32[n];
      for (int n = 0; n < H; ++n) z[n] = {frame[2 * n], frame[2 * n + 1]};
      fft_any(H, z.data(), 1, Z.data(), wH.data(), H, scratch.data());
      for (int m = 0; m < nm; ++m) mel[m] = 0.0;
      for (int k = 0; k <= H; ++k) {
        const Cpx a = Z[k % H];
        const Cpx b = {Z[(H - k) % H].re, -Z[(H - k) % H].im};
        const Cpx e = {0.5 * (a.re + b.re), 0.5 * (a.im + b.im)};
        const Cpx od = {0.5 * (a.im - b.im), -0.5 * (a.re - b.re)};
        const Cpx w = wN[k];
        const double re = e.re + od.re * w.re - od.im * w.im;
        const double im = e.im + od.re * w.im + od.im * w.re;
        const float pk = (float)(re * re + im * im);          // HF's magnitudes are fp32
        const float* v = fb.data() + (size_t)k * nm + fb_first[k];
        for (int c = 0; c < fb_count[k]; ++c) mel[fb_first[k] + c] += (double)v[c] * (double)pk;
      }
      for (int m = 0; m < nm; ++m) {
        float v = (float)mel[m];
        if (v < 1e-10f) v = 1e-10f;
        const float lg = (float)log10((double)v);
        raw[(size_t)m * live + t] = lg;
        if (lg > seg_max) seg_max = lg;
      }
    }
    if (live < frames && -10.0f > seg_max) seg_max = -10.0f;   // the dead frames' log10(1e-10) takes part in the max
    const float floor_v = seg_max - 8.0f;
    const float dead = ((-10.0f > floor_v ? -10.0f : floor_v) + 4.0f) / 4.0f;
    for (int m = 0; m < nm; ++m) {
      float* row = o + (size_t)m * frames;
      const float* r = raw.data() + (size_t)m * live;
      for (int t = 0; t < live; ++t) row[t] = ((r[t] > floor_v ? r[t] : floor_v) + 4.0f) / 4.0f;
      for (int t = live; t < frames; ++t) row[t] = dead;
    }
  }
  return GWW_OK;
}
