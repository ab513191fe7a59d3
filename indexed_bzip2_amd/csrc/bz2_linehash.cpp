/**
 * bz2_linehash.cpp -- the part of the line-hash calls of include/mi355x_bz2.h that needs no GPU (bz2_linehash.hpp).
 */
#include "../../include/mi355x_bz2.h"
#include "bz2_linehash.hpp"

extern "C" {

uint64_t
mi355x_bz2_line_hash( const uint8_t* bytes, uint64_t size, uint64_t seed )
{
    return bytes == nullptr ? 0 : bz2gpu::lineHash( bytes, (size_t)size, seed );
}

uint32_t
mi355x_bz2_line_hash_chunk_bytes( void )
{
    return bz2gpu::LINEHASH_CHUNK_BYTES;
}

}  // extern "C"
