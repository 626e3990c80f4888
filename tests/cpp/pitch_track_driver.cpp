// pitch_track_driver.cpp — melonix::PitchTrack from a compiled program (tests/test_gpu_pitch_track.py):
//   pitch_track_driver <in.f32> <sampleRate> <scaleMask> <out.markers>
// reads raw float32 samples, writes correctionMarkers(1, scaleMask) as raw Marker records.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gl_sink.hpp"
#include "pitch-track.hpp"

// the headless facade (NO_GL) leaves its few GL calls to the embedding program; this one makes no texture
extern "C" {
void glGenTextures(GLsizei, GLuint *) {}
void glDeleteTextures(GLsizei, const GLuint *) {}
void glBindTexture(GLenum, GLuint) {}
void glTexParameteri(GLenum, GLenum, GLint) {}
void glTexImage1D(GLenum, GLint, GLint, GLsizei, GLint, GLenum, GLenum, const void *) {}
}

int main(int argc, char **argv) {
  if (argc != 5) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  std::vector<float> wav;
  float buf[4096];
  size_t k;
  while ((k = std::fread(buf, sizeof(float), 4096, f)) > 0) wav.insert(wav.end(), buf, buf + k);
  std::fclose(f);
  melonix::PitchTrack track(wav, std::atoi(argv[2]));
  if (!track.ok()) return 4;
  const std::vector<Marker> mk = track.correctionMarkers(1.f, std::atoi(argv[3]));
  FILE *o = std::fopen(argv[4], "wb");
  if (!o) return 5;
  std::fwrite(mk.data(), sizeof(Marker), mk.size(), o);
  std::fclose(o);
  std::printf("%zu frames, %zu markers\n", track.frames().size(), mk.size());
  return mk.empty() ? 6 : 0;
}
