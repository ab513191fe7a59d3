/**
 * bz2_regex.cpp -- the part of the regular-expression calls of include/mi355x_bz2.h that needs no GPU: compiling a
 * pattern (bz2_regex.hpp) and handing out its table.
 */
#include <cstdio>
#include <cstring>
#include <exception>
#include <new>
#include <string>

#include "../../include/mi355x_bz2.h"
#include "bz2_ctx.hpp"
#include "bz2_regex.hpp"

static_assert( MI355X_BZ2_REGEX_MAX_STATES == bz2gpu::REGEX_MAX_STATES, "the C ABI's limit is the compiler's" );

extern "C" {

int
mi355x_bz2_regex_compile( const uint8_t* pattern, uint64_t size, uint32_t flags, mi355x_bz2_regex** re, char* error,
                          uint64_t errorCapacity )
{
    const auto say = [error, errorCapacity] ( const std::string& message ) {
        if ( error != nullptr && errorCapacity > 0 ) std::snprintf( error, (size_t)errorCapacity, "%s", message.c_str() );
    };
    say( "" );
    if ( re == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    *re = nullptr;
    if ( ( flags & ~bz2gpu::SEARCH_KNOWN_FLAGS ) != 0 ) {
        char bits[16];
        std::snprintf( bits, sizeof( bits ), "0x%X", flags & ~bz2gpu::SEARCH_KNOWN_FLAGS );
        say( std::string( "regex_compile: unknown flag bits " ) + bits );
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    if ( pattern == nullptr && size > 0 ) {
        say( "regex_compile: no pattern" );
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    try {
        auto compiled = bz2gpu::compileRegex( pattern, (size_t)size, ( flags & bz2gpu::SEARCH_IGNORE_CASE ) != 0 );
        *re = new mi355x_bz2_regex{ std::move( compiled ) };
        return MI355X_BZ2_OK;
    } catch ( const std::invalid_argument& refused ) {
        say( refused.what() );
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    } catch ( const std::bad_alloc& ) {
        say( "regex_compile: out of memory" );
        return MI355X_BZ2_ERR_DEVICE;
    } catch ( const std::exception& other ) {
        say( other.what() );
        return MI355X_BZ2_ERR_LOGIC;
    }
}

void
mi355x_bz2_regex_free( mi355x_bz2_regex* re )
{
    delete re;
}

uint32_t
mi355x_bz2_regex_states( const mi355x_bz2_regex* re )
{
    return re != nullptr ? re->dfa.n : 0;
}

int
mi355x_bz2_regex_table( const mi355x_bz2_regex* re, uint8_t* transitions, uint8_t* acceptsAtEnd )
{
    if ( re == nullptr || transitions == nullptr || acceptsAtEnd == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    std::memcpy( transitions, re->dfa.transitions.data(), re->dfa.transitions.size() );
    std::memcpy( acceptsAtEnd, re->dfa.acceptsAtEnd.data(), re->dfa.acceptsAtEnd.size() );
    return MI355X_BZ2_OK;
}

uint32_t
mi355x_bz2_regex_chunk_bytes( void )
{
    return bz2gpu::REGEX_CHUNK_BYTES;
}

}  // extern "C"
