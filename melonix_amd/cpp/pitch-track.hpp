// pitch-track.hpp — NOT in the reference (its Marker::note comes from the mouse, app.cpp:923,937): the build-defined YIN f0
// tracker (mx_f0_track), the notes cut from it (mx_detect_notes) and the markers that retune them (mx_correction_markers),
// as a class the App can own next to `spec` and its melonix::Resynth.
//
//   melonix::PitchTrack track(wavData, sampleRate);   // uploads once, tracks every frame (hop 256) on the GPU
//   markers = track.correctionMarkers(1.f, 0);          // every note onto the semitone grid ...
//   invalidateCache();                                  // ... and exportWav / renderPV retune the take;
//   resynth.exportWavPSOLA(file, markers, track.frames(), track.hop());   // or, the formants left in place, PSOLA
#pragma once
#include <cstdint>
#include <span>
#include <vector>

#include "marker.hpp"
#include "melonix_amd.h"

namespace melonix {

class PitchTrack {
public:
  // hop: samples between frame centres; fmin / fmax / threshold: the tracker's band and YIN threshold
  // decoded: frames() holds the Viterbi-decoded track (mx_f0_track_decoded, default parameters) instead of the plain one: one
  // path through each frame's candidate ladder, which does not jump an octave for a few frames where plain YIN does
  PitchTrack(std::span<const float> wav, int sampleRate, int hop = 256, float fmin = 55.f, float fmax = 1760.f,
             float threshold = 0.15f, int device = 0, bool decoded = false);

  bool ok() const { return good; }
  int hop() const { return hop_; }
  // one record per frame h (centred on sample h * hop)
  const std::vector<mx_f0> &frames() const { return track; }
  // notes with the default parameters (mx_note_params_default), or with `p`.  On a decoded track the defaults take
  // threshold = 2 x the tracker's: the decoder has made the voicing decision, and its candidates reach up to 2 theta
  std::vector<mx_note> notes() const;
  std::vector<mx_note> notes(const mx_note_params &p) const;
  // the voicing parameters Resynth::renderPSOLA / exportWavPSOLA should read this track with: the defaults
  // (mx_psola_params_default), on a decoded track with threshold = 2 x the tracker's, as notes() takes it
  mx_psola_params psolaParams() const;
  // two markers per note: strength in [0, 1], scaleMask bits 0..11 = pitch classes (A = 0), 0 = all twelve
  std::vector<Marker> correctionMarkers(float strength, int scaleMask) const;

private:
  int sampleRate, hop_;
  float threshold_;
  bool decoded_;
  bool good = false;
  std::vector<mx_f0> track;
};

}  // namespace melonix
