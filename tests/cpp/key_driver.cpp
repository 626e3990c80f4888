// key_driver.cpp — melonix::KeyTrack from a compiled program (tests/test_gpu_key_facade.py):
//   key_driver <in.f32> <sampleRate> <notes.bin> <strength> <chroma.bin> <key.bin> <windows.bin> <markers.bin>
// reads raw float32 samples and mx_note records, writes the chroma records, the take's mx_key, the mx_key_window records of
// windows of 48 frames every 24 and the correction markers of the notes on the detected scale and grid.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "driver_common.hpp"
#include "key-track.hpp"
#include "melonix_amd.h"

int main(int argc, char **argv) {
  if (argc != 9) return 2;
  std::vector<float> wav;
  if (!read_f32(argv[1], wav)) return 3;
  const int sr = std::atoi(argv[2]);
  std::vector<mx_note> notes;
  {
    FILE *f = std::fopen(argv[3], "rb");
    if (!f) return 3;
    mx_note n;
    while (std::fread(&n, sizeof n, 1, f) == 1) notes.push_back(n);
    std::fclose(f);
  }
  const float strength = (float)std::atof(argv[4]);
  const melonix::KeyTrack track(wav, sr, 2048, 48, 24);
  if (!track.ok()) return 4;
  const std::vector<Marker> markers = track.correctionMarkers(notes, strength);
  if (track.keyWindows().empty() || markers.size() != 2 * notes.size()) return 5;
  if (!dump(argv[5], track.chroma()) || !dump(argv[6], std::vector<mx_key>{track.key()}) || !dump(argv[7], track.keyWindows()) ||
      !dump(argv[8], markers))
    return 6;
  // no windows asked for: none; a failed call gives empty results and a zero key
  const melonix::KeyTrack plain(wav, sr);
  if (!plain.ok() || !plain.keyWindows().empty() || plain.key().tonic != track.key().tonic || plain.chroma().size() != track.chroma().size()) return 7;
  if (!track.correctionMarkers(notes, 1.5f).empty()) return 8;
  std::vector<mx_note> swapped(notes.rbegin(), notes.rend());
  if (notes.size() > 1 && !track.correctionMarkers(swapped, strength).empty()) return 9;
  if (!track.correctionMarkers({}, strength).empty()) return 10;  // (no notes: no markers)
  for (const melonix::KeyTrack &none : {melonix::KeyTrack(wav, sr, 0), melonix::KeyTrack(wav, 0), melonix::KeyTrack(wav, sr, 2048, 48, 0)})
    if (none.ok() || !none.chroma().empty() || !none.keyWindows().empty() || none.key().scale_mask != 0 || none.key().tuning_cents != 0.0 ||
        !none.correctionMarkers(notes, strength).empty())
      return 11;
  std::printf("%zu frames, %zu windows, tonic %d mode %d\n", track.chroma().size(), track.keyWindows().size(), track.key().tonic, track.key().mode);
  return 0;
}
