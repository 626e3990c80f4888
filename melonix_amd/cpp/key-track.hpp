// key-track.hpp — NOT in the reference (it has no detector): the build-defined key, scale and tuning estimate (mx_chroma,
// mx_key_detect) and the correction markers on the detected grid (mx_correction_markers_tuned), as a class the App can own
// next to its melonix::PitchTrack.  Give it what says most about the key: the accompaniment or the mix rather than the dry take.
//
//   melonix::KeyTrack key(mixData, sampleRate);                       // uploads once: chroma records, window sums, the key
//   // "Detect key and tuning": key.key().tonic / .mode / .tuning_cents, key.key().clarity to decide whether to believe it
//   markers = key.correctionMarkers(track.notes(), 1.f);              // "Auto-correct pitch" on that scale and that grid
#pragma once
#include <cstdint>
#include <span>
#include <vector>

#include "marker.hpp"
#include "melonix_amd.h"

namespace melonix {

class KeyTrack {
public:
  // hop: samples between frame centres (key needs no fine grid).  windowFrames > 0: a key per window of that many frames,
  // every windowHop frames, beside the take's.  The chroma parameters are the library's defaults.
  KeyTrack(std::span<const float> wav, int sampleRate, int hop = 2048, int windowFrames = 0, int windowHop = 1, int device = 0);

  bool ok() const { return good; }
  int hop() const { return hop_; }
  // the record of frame h (centred on sample h * hop); empty after a failed call
  const std::vector<mx_chroma_rec> &chroma() const { return chroma_; }
  // the take's key; all zero (scale_mask 0: "don't know") after a failed call
  const mx_key &key() const { return key_; }
  // one key per window; empty after a failed call and without windows
  const std::vector<mx_key_window> &keyWindows() const { return windows_; }
  // two markers per note, each note moved onto key()'s scale on key()'s grid; empty after a failed call
  std::vector<Marker> correctionMarkers(const std::vector<mx_note> &notes, float strength) const;

private:
  int hop_;
  bool good = false;
  std::vector<mx_chroma_rec> chroma_;
  mx_key key_{};
  std::vector<mx_key_window> windows_;
};

}  // namespace melonix
