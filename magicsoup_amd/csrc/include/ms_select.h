// Single-source probabilistic selection shared by the OpenMP host path and the HIP kernels
// (World.kill_divide_prob): the Hill curves of the kill / divide probabilities, one Philox4x32-10
// block per cell for their four uniforms, and the per-cell decision.
//
// Everything is fp32 in the written operation order, with IEEE divisions, so the g++ build and the
// gfx950 build (-ffp-contract=off) decide every cell alike.
#pragma once
#include <stdint.h>

#include "ms_kinetics.h"

namespace ms {

// One Philox4x32-10 block: counter (c0, c1, c2, c3), key (k0, k1) -> out[0..3] in output order (the
// round function of msd::Philox::next, on plain words).
MS_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
  uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = c3, a = k0, b = k1;
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * x0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * x2;
    const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ a;
    const uint32_t y2 = (uint32_t)(p0 >> 32) ^ x3 ^ b;
    x1 = (uint32_t)p1;
    x3 = (uint32_t)p0;
    x0 = y0;
    x2 = y2;
    a += 0x9E3779B9u;
    b += 0xBB67AE85u;
  }
  out[0] = x0;
  out[1] = x1;
  out[2] = x2;
  out[3] = x3;
}

// The four uniforms in [0, 1) of cell `item` in the call (seed, call): the first block of
// msd::Philox(seed, call, item), i.e. four successive uniform() calls.
MS_HD void selection_uniforms(uint64_t seed, uint64_t call, uint32_t item, float u[4]) {
  uint32_t w[4];
  philox4x32_10(item, (uint32_t)call, (uint32_t)(call >> 32), 0u, (uint32_t)seed, (uint32_t)(seed >> 32), w);
  for (int j = 0; j < 4; ++j) u[j] = (float)(w[j] >> 8) * (1.0f / 16777216.0f);
}

// Hill curves over v with half-saturation K and integer exponent n.
// rise: 0 -> 1 as v grows; NaN and v <= 0 -> 0, +inf -> 1
MS_HD float rise(float v, float K, int n) { return v > 0.0f ? 1.0f / (1.0f + ipow(K / v, n)) : 0.0f; }
// fall: 1 -> 0 as v grows; NaN and v <= 0 -> 1, +inf -> 0
MS_HD float fall(float v, float K, int n) { return v > 0.0f ? 1.0f / (1.0f + ipow(v / K, n)) : 1.0f; }

// The rule of one kill_divide_prob call (passed to kernels by value).
struct SelectRule {
  int32_t mol;                     // the molecule the kill / divide terms read
  float kill_k, divide_k, genome_k;
  int32_t kill_n, divide_n, genome_n;
  uint32_t enable;                 // kSelKill | kSelDivide | kSelGenome
  float cost;                      // paid from `mol` by a dividing cell
  float kill_fraction;             // unconditional kill probability (dilution)
};
constexpr uint32_t kSelKill = 1u, kSelDivide = 2u, kSelGenome = 4u;

// A cell's decision from its molecule x, genome length g and four uniforms: bit 0 kill, bit 1 divide.
// All four uniforms belong to fixed terms (u0 dilution, u1 molecule kill, u2 genome kill, u3
// division), so enabling a term never changes the draws of the others.
MS_HD int select_decide(const SelectRule& r, float x, float g, const float u[4]) {
  bool k = u[0] < r.kill_fraction;
  if (r.enable & kSelKill) k |= u[1] < fall(x, r.kill_k, r.kill_n);
  if (r.enable & kSelGenome) k |= u[2] < rise(g, r.genome_k, r.genome_n);
  const bool d = !k && (r.enable & kSelDivide) && u[3] < rise(x, r.divide_k, r.divide_n);
  return (k ? 1 : 0) | (d ? 2 : 0);
}

}  // namespace ms
