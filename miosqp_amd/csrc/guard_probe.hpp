// The probe vectors of the inverse guard (kernels_guard.inc), as one function every user of them shares: the guard
// kernels of a single engine and the one-launch set-up of many models (setup_models_body.hpp).  Plain C++ with the
// HIP qualifiers only under hipcc, so that the stand-alone CPU programs under tests/ read the same entries.
#pragma once

#if defined(__HIPCC__)
#define MIOSQP_HD __host__ __device__
#else
#define MIOSQP_HD
#endif

namespace miosqp {

// entry c of probe vector p: fixed pseudo-random, in [-1, 1)
MIOSQP_HD inline double guard_probe_value(int p, int c) {
  unsigned h = (unsigned)(c + 1) * 2654435761u ^ (unsigned)(p + 1) * 0x9E3779B9u;
  h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
  return (double)(int)(h & 0xFFFFFu) / 524288.0 - 1.0;
}

}  // namespace miosqp
