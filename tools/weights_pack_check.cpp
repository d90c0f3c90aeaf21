// weights_pack_check.cpp -- the weight blob's host twin,
// mzgo_weights_pack_host (csrc/mzgo_weights.hip), called from a stand-alone
// host program so that the host walk of the pack plan -- the decoded indices it
// reads the tensors through, the writes into the caller's blob -- can run under
// AddressSanitizer and UBSan on a machine without a GPU.  The program links the
// weights unit alone: what that unit takes from mzgo_capi.hip is stubbed below,
// and no HIP call is made.  Every tensor and every blob has exactly the size
// the header promises, so a read or write past it is a report.  For each of the
// six kernel sets the blob is packed twice: from tensors without a zero, into a
// blob pre-filled with a marker, to see that every float inside a part's
// unpadded length holds a source float -- or the zero the rules put into the
// MG == 3 pad slot and conv1's padded input channels, which are counted against
// the layout -- and every float outside is zero; and from zero tensors, to see
// that nothing but zeros comes out.  Exit status 0 and "ok" = clean.
//
// Build and run (host code sanitized, device code as the library's):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off \
//     -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//     -x hip tools/weights_pack_check.cpp muzero-go_amd/csrc/mzgo_weights.hip -o tools/weights_pack_check
//   tools/weights_pack_check
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/mzgo.h"
#include "../muzero-go_amd/csrc/mzgo_weights.hpp"

using namespace mzgo;

// ---- mzgo_capi.hip's side of the weights unit, stubbed ----
static std::string g_err;
int mzgo::set_error(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
static const int kSets[6][2] = {{5, 96}, {6, 64}, {6, 96}, {6, 128}, {9, 96}, {19, 96}};
const KernelSet* mzgo::find_kernels(int N, int C) {
  for (const auto& s : kSets)
    if (s[0] == N && s[1] == C) return reinterpret_cast<const KernelSet*>(&kSets);   // (non-null: never read)
  return nullptr;
}

#define CHECK(c)                                                            \
  do {                                                                      \
    if (!(c)) {                                                             \
      fprintf(stderr, "%s:%d: %s (%s)\n", __FILE__, __LINE__, #c, g_err.c_str()); \
      return 1;                                                             \
    }                                                                       \
  } while (0)

int main() {
  long floats = 0, rule_zeros = 0;
  for (const auto& set : kSets) {
    const int N = set[0], C = set[1], A = N * N + 1;
    const WeightLayout L = weight_layout(N, C, A);
    // the 22 tensors, each exactly its shape's floats
    std::vector<std::vector<float>> t(WK_COUNT);
    const char* keys[WK_COUNT];
    const float* data[WK_COUNT];
    const int64_t* shapes[WK_COUNT];
    int64_t dims[WK_COUNT][4];
    int ndims[WK_COUNT];
    for (int k = 0; k < WK_COUNT; ++k) {
      const WeightShape sh = weight_key_shape(k, C, A);
      size_t n = 1;
      for (int d = 0; d < sh.nd; ++d) n *= (size_t)(dims[k][d] = sh.d[d]);
      t[k].resize(n);
      keys[k] = kWeightKeyNames[k];
      shapes[k] = dims[k];
      ndims[k] = sh.nd;
    }
    int64_t total = -1;
    for (int pass = 0; pass < 2; ++pass) {
      // pass 0: positive values (the tap table's and the Winograd sums of
      // positive terms would still cancel through G's negative entries: the
      // values grow by 1/8 per element and 7 per tensor, and the sums are
      // checked against zero below); pass 1: all zero
      for (int k = 0; k < WK_COUNT; ++k) {
        for (size_t i = 0; i < t[k].size(); ++i) t[k][i] = pass ? 0.f : 1.f + 7.f * k + 0.125f * (float)(i % 4093);
        data[k] = t[k].data();
      }
      CHECK(mzgo_weights_pack_host(N, C, keys, data, shapes, ndims, WK_COUNT, nullptr, 0, &total) == MZGO_OK);
      CHECK(total == (int64_t)L.total);
      const float marker = -12345.f;
      std::vector<float> blob((size_t)total, marker);        // exactly n_floats
      CHECK(mzgo_weights_pack_host(N, C, keys, data, shapes, ndims, WK_COUNT, blob.data(), total, &total) == MZGO_OK);
      // the zeros the rules themselves write inside a part
      size_t want_zeros = conv_pack_geo(64, 6).floats / 4;   // conv1: input channels 6, 7 of 8
      const int latent[3][2] = {{64, 64}, {C, 64}, {C, C}};
      for (const auto& cc : latent) {
        const ConvPackGeo g = conv_pack_geo(cc[0], cc[1]);
        if (!L.wino && g.MG == 3) want_zeros += g.floats / 4;   // the pad slot mi == 3
      }
      size_t zeros = 0;
      for (int p = 0; p < WP_COUNT; ++p) {
        const size_t end = p + 1 < WP_COUNT ? L.off[p + 1] : L.total;
        for (size_t i = L.off[p]; i < end; ++i) {
          CHECK(blob[i] != marker);                            // written (or zeroed) by the call
          if (i >= L.off[p] + L.size[p] || pass) CHECK(blob[i] == 0.f && !std::signbit(blob[i]));
          else if (blob[i] == 0.f) {
            CHECK(p == WP_CONV1_W || p == WP_CONV2_W || p == WP_CONV3_W || p == WP_DYN_W);
            ++zeros;
          }
          ++floats;
        }
      }
      if (!pass) CHECK(zeros == want_zeros);
      if (!pass) rule_zeros += (long)zeros;
      // one float short: refused, nothing written
      std::vector<float> small((size_t)total - 1, marker);
      CHECK(mzgo_weights_pack_host(N, C, keys, data, shapes, ndims, WK_COUNT, small.data(), total - 1, &total) ==
            MZGO_EINVAL);
      for (float x : small) CHECK(x == marker);
    }
    // the table's refusals
    CHECK(mzgo_weights_pack_host(N, C, keys, data, shapes, ndims, WK_COUNT - 1, nullptr, 0, &total) == MZGO_EINVAL);
    CHECK(g_err.find("missing weight") != std::string::npos);
    keys[1] = keys[0];
    CHECK(mzgo_weights_pack_host(N, C, keys, data, shapes, ndims, WK_COUNT, nullptr, 0, &total) == MZGO_EINVAL);
    CHECK(g_err.find("duplicate key") != std::string::npos);
    CHECK(mzgo_weights_pack_host(N + 2, C, keys, data, shapes, ndims, WK_COUNT, nullptr, 0, &total) == MZGO_EINVAL);
    CHECK(g_err.find("no kernels built") != std::string::npos);
  }
  printf("ok: %ld floats over 6 kernel sets x 2 passes, %ld zeros from the rules\n", floats, rule_zeros);
  return 0;
}
