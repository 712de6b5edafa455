// gp_key_table.hpp -- THE open-addressing table of 64-bit keys: `mask + 1` slots (a power of two), kEmptyKey for a free slot, linear probing from a home slot the
// caller hashes (hash_key: the hashed k-NN grid of gp_knn.hip and the FPFH grid of gp_fpfh.hip; occ_hash: the occupancy set of gp_occupancy.hpp).  One find and one
// claim for the three tables.
//
// EVERY probe loop stops when it is back at its home slot, i.e. after at most mask + 1 probes: a damaged table (no free slot, a key stored twice) gives a wrong answer,
// never a spin.  The tables' builders keep the load at or below one half, so a free slot ends every probe long before that.
// No HIP header is needed: a host compiler builds this file alone and runs the same loops (tests/key_table_cases.cpp); the one device-specific line is key_cas.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GP_KEY_HD __host__ __device__ __forceinline__
#else
#define GP_KEY_HD inline
#endif

// one per slot read by key_find / key_claim: nothing in the library; tests/key_table_cases.cpp counts the probes through it
#ifndef GP_KEY_PROBE
#define GP_KEY_PROBE() ((void)0)
#endif

namespace gp {

constexpr unsigned long long kEmptyKey = ~0ull;  // no key of any table has bit 63 set

GP_KEY_HD uint32_t hash_key(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (uint32_t)k;
}

// stores `key` in the free slot s; returns what the slot held (kEmptyKey: stored).  Atomic on the device; on the host the plain sequence (one thread: the tests)
GP_KEY_HD unsigned long long key_cas(unsigned long long* keys, uint32_t s, unsigned long long key) {
#if defined(__HIP_DEVICE_COMPILE__)
  return atomicCAS(&keys[s], kEmptyKey, key);
#else
  const unsigned long long old = keys[s];
  if (old == kEmptyKey) keys[s] = key;
  return old;
#endif
}

// the slot that holds `key`, or -1.  (keys and mask by reference: a search kernel whose table sits in a structure it indexes per lane reads them where the loop
// uses them, as its own loop did, and holds no registers for them across the probe -- by value, covariance_kernel<10, 4, false, true> spills 10 registers for 8 and tests/test_covariance_build_cpu.py fails: do not "tidy" the signature)
GP_KEY_HD int key_find(const unsigned long long* const& keys, const uint32_t& mask, uint32_t home, unsigned long long key) {
  uint32_t s = home;
  do {
    GP_KEY_PROBE();
    const unsigned long long k = keys[s];
    if (k == key) return (int)s;
    if (k == kEmptyKey) return -1;
    s = (s + 1) & mask;
  } while (s != home);  // back at the home slot: mask + 1 probes, no free slot and no match
  return -1;
}

// the slot of `key`, claimed if it is new (*claimed = 1); mask + 1 when the table has no room.
// Claim form: a plain read first, the compare-and-swap only on a slot seen empty (a slot only ever goes from empty to a key, so a stale read costs one failed swap and
// nothing else).  Most points of a grid find their cell's key already stored and take no atomic at all.  Measured on this very code with only these lines
// exchanged (profiles/spatial_keying_time.json, tags C*): swap first, the hashed k-NN grid of 1 M points builds in 2.2 ms (as the parent's) and a 1 M-point
// occupancy insert takes 0.51 ms; read first, 1.82 ms and 0.37 ms; FPFH is the same with either.
GP_KEY_HD uint32_t key_claim(unsigned long long* keys, uint32_t mask, uint32_t home, unsigned long long key, int* claimed) {
  uint32_t s = home;
  *claimed = 0;
  do {
    GP_KEY_PROBE();
    unsigned long long k = keys[s];
    if (k == kEmptyKey) {
      k = key_cas(keys, s, key);
      if (k == kEmptyKey) {
        *claimed = 1;
        return s;
      }
    }
    if (k == key) return s;
    s = (s + 1) & mask;
  } while (s != home);  // back at the home slot: mask + 1 probes
  return mask + 1;
}

}  // namespace gp
#undef GP_KEY_HD
#undef GP_KEY_PROBE
