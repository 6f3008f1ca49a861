// blake2sp.hpp -- launch interface of the per-chunk BLAKE2sp kernel
// (blake2sp.hip); called by HashEngine (hash_engine.cpp).
#pragma once
#include "sha256.hpp"

namespace cdc {

// The batch description of launch_sha256; digests[8*k .. 8*k+8) (u32,
// little-endian bytes) = BLAKE2sp-256 of chunk k, unkeyed.
hipError_t launch_blake2sp(const ShaBatch &b, int num_cus, hipStream_t s);

}  // namespace cdc
