/**
 * bz2_fields.cpp -- the part of the field calls of include/mi355x_bz2.h that needs no GPU (bz2_fields.hpp).
 */
#include "../../include/mi355x_bz2.h"
#include "bz2_fields.hpp"
#include "bz2_fieldcols.hpp"

extern "C" {

uint32_t
mi355x_bz2_field_chunk_bytes( void )
{
    return bz2gpu::FIELD_CHUNK_BYTES;
}

uint32_t
mi355x_bz2_gather_fields_tile_bytes( void )
{
    return bz2gpu::FIELD_COLUMN_TILE_BYTES;
}

}  // extern "C"
