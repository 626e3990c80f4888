// f0_notes.cpp — notes and correction markers from a YIN track (definitions: include/melonix_amd.h).  Pure host code,
// built with g++ -ffp-contract=off: tests/test_f0_host.py restates it in Python and expects the same doubles.
#include "f0_notes.h"

#include <cmath>
#include <functional>
#include <queue>
#include <vector>

namespace mx {

double period_note(double period, int sampleRate) { return 24.0 + 12.0 * std::log2((double)sampleRate / period / 55.0); }

namespace {

// running median of a run: the lower half in a max-heap, the upper half in a min-heap (lo holds the extra element)
struct RunMedian {
  std::priority_queue<double> lo;
  std::priority_queue<double, std::vector<double>, std::greater<double>> hi;
  void clear() {
    lo = {};
    hi = {};
  }
  void push(double v) {
    if (lo.empty() || v <= lo.top()) lo.push(v);
    else hi.push(v);
    if (lo.size() > hi.size() + 1) {
      hi.push(lo.top());
      lo.pop();
    } else if (hi.size() > lo.size()) {
      lo.push(hi.top());
      hi.pop();
    }
  }
  double median() const { return lo.size() > hi.size() ? lo.top() : (lo.top() + hi.top()) / 2.0; }
};

}  // namespace

std::vector<mx_note> detect_notes(const mx_f0 *track, int64_t count, int sampleRate, int hop, int64_t first_frame,
                                  const mx_note_params &p) {
  std::vector<mx_note> out;
  std::vector<double> m((size_t)count);
  RunMedian med;
  int64_t start = -1;  // first frame of the open run (-1: none)
  auto close = [&](int64_t end) {  // frames [start, end)
    if (start >= 0 && end - start >= p.min_frames) {
      mx_note n{};
      n.first_frame = (int32_t)(first_frame + start);
      n.frames = (int32_t)(end - start);
      n.start_sample = (int32_t)((first_frame + start) * hop);
      n.end_sample = (int32_t)((first_frame + end - 1) * hop);
      n.note = med.median();
      double ap = 0.0, spread = 0.0;
      for (int64_t f = start; f < end; ++f) {
        ap += (double)track[f].aperiodicity;
        const double dv = std::fabs(m[(size_t)f] - n.note);
        spread = dv > spread ? dv : spread;
      }
      n.aperiodicity = (float)(ap / (double)(end - start));
      n.spread = (float)spread;
      out.push_back(n);
    }
    start = -1;
    med.clear();
  };
  for (int64_t f = 0; f < count; ++f) {
    const mx_f0 &r = track[f];
    const bool voiced = r.tau > 0 && r.aperiodicity < p.threshold && r.rms >= p.rms_floor;
    if (!voiced) {
      close(f);
      continue;
    }
    m[(size_t)f] = period_note((double)r.period, sampleRate);
    if (start >= 0 && (std::fabs(m[(size_t)f] - m[(size_t)f - 1]) > p.max_jump || std::fabs(m[(size_t)f] - med.median()) > p.max_dev))
      close(f);
    if (start < 0) start = f;
    med.push(m[(size_t)f]);
  }
  close(count);
  return out;
}

double snap_note(double note, int mask) {
  const double base = std::floor(note);
  double best = 0.0, bestd = HUGE_VAL;
  for (int k = -12; k <= 13; ++k) {  // every pitch class occurs on each side within 12 semitones
    const double c = base + k;
    const int cls = (int)(((int64_t)c % 12 + 12) % 12);
    if (mask && !((mask >> cls) & 1)) continue;
    const double d = std::fabs(c - note);
    if (d < bestd) {
      bestd = d;
      best = c;
    }
  }
  return best;
}

void correction_markers(const mx_note *notes, int64_t count, double strength, int mask, mx_marker *out) {
  for (int64_t i = 0; i < count; ++i) {
    const mx_note &n = notes[i];
    const double b = strength * (snap_note(n.note, mask) - n.note);
    out[2 * i] = mx_marker{n.start_sample, n.note, 0.0, b};
    out[2 * i + 1] = mx_marker{n.end_sample, n.note, 0.0, b};
  }
}

}  // namespace mx
