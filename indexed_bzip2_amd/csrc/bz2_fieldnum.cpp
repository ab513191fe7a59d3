/**
 * bz2_fieldnum.cpp -- the part of the field-number calls of include/mi355x_bz2.h that needs no GPU (bz2_fieldnum.hpp).
 */
#include "../../include/mi355x_bz2.h"
#include "bz2_fieldnum.hpp"

static_assert( bz2gpu::FIELD_NOT_A_NUMBER == MI355X_BZ2_FIELD_NOT_A_NUMBER && bz2gpu::FIELD_NUMBER_MISSING == MI355X_BZ2_FIELD_NUMBER_MISSING,
               "the C ABI's constants" );

extern "C" {

int64_t
mi355x_bz2_parse_field_number( const uint8_t* bytes, uint64_t size )
{
    if ( bytes == nullptr ) return bz2gpu::FIELD_NOT_A_NUMBER;
    return bz2gpu::parseFieldNumber( bytes, size );
}

}  // extern "C"
