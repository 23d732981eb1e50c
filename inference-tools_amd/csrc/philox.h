// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11 - the Random123
// generator) and the map from one of its blocks to the two uniforms of a pair of normal variates.  Integer code only, shared
// by the device generator (draws.hip: draws_normals_kernel) and the host entry point gpmi_draws_normals, so both walk the
// same stream; tests/draws_host.py is its NumPy mirror.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define GPMI_HD __host__ __device__
#else
#define GPMI_HD
#endif

struct PhiloxBlock {
  uint32_t r[4];
};

// one round: (c0, c1, c2, c3) -> (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
GPMI_HD inline PhiloxBlock philox_round(const PhiloxBlock& c, uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c.r[0], p1 = (uint64_t)0xCD9E8D57u * c.r[2];
  return {{(uint32_t)(p1 >> 32) ^ c.r[1] ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.r[3] ^ k1, (uint32_t)p0}};
}

// ten rounds; the key takes one Weyl step between rounds
GPMI_HD inline PhiloxBlock philox4x32_10(PhiloxBlock c, uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    c = philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// The block of columns 2 p and 2 p + 1 of draw s: key = the two halves of the seed's 64-bit pattern, counter = (p, s, 0).
// Its words give u1 in (0, 1] and u2 in [0, 1) as 53-bit integers n1 in [1, 2^53], n2 in [0, 2^53): u = n 2^-53, exact.
GPMI_HD inline void draws_uniform_bits(uint64_t seed, uint64_t s, uint32_t p, uint64_t& n1, uint64_t& n2) {
  const PhiloxBlock b = philox4x32_10({{p, (uint32_t)s, (uint32_t)(s >> 32), 0u}}, (uint32_t)seed, (uint32_t)(seed >> 32));
  n1 = ((uint64_t)(b.r[0] >> 5) << 26) + (uint64_t)(b.r[1] >> 6) + 1u;
  n2 = ((uint64_t)(b.r[2] >> 5) << 26) + (uint64_t)(b.r[3] >> 6);
}

constexpr double DRAWS_TWO_PI = 6.283185307179586;  // fl(2 pi) = 0x401921FB54442D18
constexpr double DRAWS_2M53 = 1.0 / 9007199254740992.0;
