// pitch_track_decoded_driver.cpp — melonix::PitchTrack's `decoded` option from a compiled program
// (tests/test_gpu_f0_decode.py):
//   pitch_track_decoded_driver <in.f32> <sampleRate> <decoded 0|1> <out.frames>
// reads raw float32 samples, writes frames() as raw mx_f0 records and prints the number of notes() on its last line.
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
  melonix::PitchTrack track(wav, std::atoi(argv[2]), 256, 55.f, 1760.f, 0.15f, 0, std::atoi(argv[3]) != 0);
  if (!track.ok()) return 4;
  FILE *o = std::fopen(argv[4], "wb");
  if (!o) return 5;
  std::fwrite(track.frames().data(), sizeof(mx_f0), track.frames().size(), o);
  std::fclose(o);
  std::printf("notes %zu\n", track.notes().size());
  return 0;
}
