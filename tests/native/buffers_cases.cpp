/* The planner of mi355x_bz2_decompress_buffers (bz2_buffers.hpp) against a plain restatement.  Buffers are built bit by
 * bit from a list of items (stream headers, data blocks at any bit offset, end-of-stream blocks with their stored CRC,
 * garbage), packed, scanned for the block magic by brute force, and decoded by a fake launch that lays out each
 * launch's blocks back to back as the GPU does.  The chain walk's results and the bytes its pieces put in place are
 * compared with what the item list says: statuses and error offsets, blocks, streams, trailing garbage, output offsets
 * (failed buffers take 0 bytes).  Cases: windows at and around the budget, matches that straddle two buffers, launch caps
 * 1, 2, 7 and 512 with buffers spanning launches, multi-stream chains, trailing garbage, a false-positive magic inside a
 * block, a damaged magic (behind a block: ERR_BAD_MAGIC; as a stream's first block: ERR_BAD_MAGIC only if a block magic
 * follows in the buffer, else the buffer ends there, as the reader's scan-driven walk does), a stream-CRC mismatch, a
 * failed block inside a multi-block buffer, an empty buffer, a cut inside an end-of-stream block; plus seeded mixtures
 * under several seeds.  Prints "buffers ok". */
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_buffers.hpp"

using namespace mi355x::buffers;

namespace
{
int failures = 0;
const char* currentCase = "";

#define CHECK( cond )                                                                          \
    do {                                                                                       \
        if ( !( cond ) ) {                                                                     \
            if ( failures < 20 ) std::printf( "FAILED line %d (%s): %s\n", __LINE__, currentCase, #cond ); \
            ++failures;                                                                        \
        }                                                                                      \
    } while ( 0 )

struct Bits
{
    std::vector<uint8_t> bytes;
    uint64_t n{ 0 };
    void put( uint64_t value, unsigned count )
    {
        for ( unsigned i = count; i-- > 0; ) {
            if ( n % 8 == 0 ) bytes.push_back( 0 );
            if ( ( value >> i ) & 1u ) bytes.back() |= (uint8_t)( 0x80u >> ( n % 8 ) );
            ++n;
        }
    }
    void pad() { while ( n % 8 != 0 ) put( 0, 1 ); }
};

/* a data block as the fake decoder sees it */
struct Block
{
    uint64_t bits{ 0 }, length{ 0 }, decoded{ 0 };
    uint32_t crc{ 0 };
    int32_t status{ MI355X_BZ2_OK };
};

/* one buffer: its bytes, the real blocks (by bit offset) and the expected result */
struct Spec
{
    Bits data;
    std::map<uint64_t, Block> blocks;
    BufferResult want;
    std::vector<std::pair<uint64_t, uint64_t> > pieces;   /* expected output: (block bits, decoded size) in order */
    /* A damaged magic right behind a stream header: the reader takes the next block its scan found and ends the file
     * without complaint if there is none.  So `want` (ERR_BAD_MAGIC) holds only if a block magic lies at or behind
     * `endsOkAt` in this buffer; otherwise the buffer ends there with `okWant` and `okPieces`. */
    uint64_t endsOkAt{ UINT64_MAX };
    BufferResult okWant;
    std::vector<std::pair<uint64_t, uint64_t> > okPieces;
};

struct Builder
{
    Spec s;
    uint32_t fold{ 0 };
    bool failed{ false };
    bool afterHeader{ false };   /* the next block is the first of its stream */
    std::mt19937_64& rng;
    explicit Builder( std::mt19937_64& r ) : rng( r ) {}

    void fail( int32_t status, uint64_t at )
    {
        if ( failed ) return;
        failed = true;
        s.want.status = status;
        s.want.errorOffsetBits = at;
        s.want.decodedSize = 0;
        s.pieces.clear();
    }
    void header( char level = '9' )
    {
        s.data.put( 'B', 8 );
        s.data.put( 'Z', 8 );
        s.data.put( 'h', 8 );
        s.data.put( (uint8_t)level, 8 );
        afterHeader = true;
    }
    /* a data block of `payload` bits behind magic and CRC; `fakeMagicAt`: a block magic inside its payload */
    void block( uint64_t payload, uint64_t decoded, int32_t status = MI355X_BZ2_OK, bool fakeMagic = false,
                bool damagedMagic = false )
    {
        Block b;
        b.bits = s.data.n;
        b.length = 80 + payload;
        b.decoded = decoded;
        b.crc = (uint32_t)rng();
        b.status = status;
        s.data.put( damagedMagic ? MI355X_BZ2_MAGIC_BLOCK ^ 0x10000 : MI355X_BZ2_MAGIC_BLOCK, 48 );
        s.data.put( b.crc, 32 );
        for ( uint64_t i = 0; i < payload; ) {
            if ( fakeMagic && i == payload / 2 && payload - i > 48 ) {
                s.data.put( MI355X_BZ2_MAGIC_BLOCK, 48 );
                i += 48;
                continue;
            }
            const unsigned k = (unsigned)std::min<uint64_t>( 16, payload - i );
            s.data.put( rng() & 0x7777u & ( ( 1u << k ) - 1 ), k );   /* never six ones in a row: no magic by accident */
            i += k;
        }
        const bool first = afterHeader;
        afterHeader = false;
        if ( damagedMagic ) {
            if ( first && !failed ) {
                s.endsOkAt = b.bits;
                s.okWant = s.want;
                s.okPieces = s.pieces;
            }
            fail( MI355X_BZ2_ERR_BAD_MAGIC, b.bits );
            return;
        }
        s.blocks[b.bits] = b;
        if ( status != MI355X_BZ2_OK ) {
            fail( status, b.bits );
            return;
        }
        if ( failed ) return;
        fold = ( ( fold << 1 ) | ( fold >> 31 ) ) ^ b.crc;
        s.want.blocks += 1;
        s.want.decodedSize += decoded;
        if ( decoded > 0 ) s.pieces.push_back( { b.bits, decoded } );
    }
    void eos( bool wrongCrc = false )
    {
        const uint64_t at = s.data.n;
        s.data.put( MI355X_BZ2_MAGIC_EOS, 48 );
        s.data.put( wrongCrc ? fold ^ 1u : fold, 32 );
        s.data.pad();
        afterHeader = false;
        if ( wrongCrc ) fail( MI355X_BZ2_ERR_STREAM_CRC, at );
        if ( !failed ) s.want.streams += 1;
        fold = 0;
    }
    void garbage( size_t bytes )
    {
        for ( size_t i = 0; i < bytes; ++i ) s.data.put( 0x5A ^ ( i & 0x1F ), 8 );
        if ( !failed ) s.want.trailingGarbage = true;
    }
};

/* decoded byte j of the block at `bits` of buffer `b` */
uint8_t decodedByte( uint32_t b, uint64_t bits, uint64_t j ) { return (uint8_t)( b * 131 + bits * 7 + j * 13 ); }

/* the brute-force scan: every bit offset of the block magic in the packed bytes */
std::vector<uint64_t>
scan( const std::vector<uint8_t>& packed )
{
    std::vector<uint64_t> found;
    const uint64_t nBits = 8 * packed.size();
    for ( uint64_t p = 0; p + 48 <= nBits; ++p ) {
        uint64_t v = 0;
        for ( unsigned i = 0; i < 48; ++i ) v = ( v << 1 ) | ( ( packed[( p + i ) >> 3] >> ( 7 - ( ( p + i ) & 7 ) ) ) & 1u );
        if ( v == MI355X_BZ2_MAGIC_BLOCK ) found.push_back( p );
    }
    return found;
}

/* runs the planner over the buffers (one window) with launch cap `cap` and checks everything against the specs */
void
runCase( const char* name, std::vector<Spec>& specs, uint32_t cap, std::mt19937_64& rng )
{
    currentCase = name;
    const uint32_t n = (uint32_t)specs.size();
    std::vector<uint64_t> sizes( n );
    std::vector<const uint8_t*> data( n );
    std::vector<uint8_t> packed;
    for ( uint32_t b = 0; b < n; ++b ) {
        sizes[b] = specs[b].data.bytes.size();
        data[b] = specs[b].data.bytes.data();
        packed.insert( packed.end(), specs[b].data.bytes.begin(), specs[b].data.bytes.end() );
    }
    const auto matches = scan( packed );
    const WindowPlan plan = planWindow( sizes.data(), n, matches.data(), matches.size(), cap );

    /* candidates: every match that lies wholly in one buffer, with that buffer's end; launches of at most cap */
    size_t expectCandidates = 0;
    for ( const auto m : matches ) {
        uint64_t start = 0;
        for ( uint32_t b = 0; b < n; ++b ) {
            const uint64_t end = start + sizes[b];
            if ( m >= 8 * start && m < 8 * end ) {
                if ( m + 48 <= 8 * end ) {
                    CHECK( expectCandidates < plan.bits.size() && plan.bits[expectCandidates] == m );
                    CHECK( expectCandidates < plan.endBytes.size() && plan.endBytes[expectCandidates] == end );
                    CHECK( expectCandidates < plan.buffer.size() && plan.buffer[expectCandidates] == b );
                    ++expectCandidates;
                }
                break;
            }
            start = end;
        }
    }
    CHECK( plan.bits.size() == expectCandidates );
    const uint32_t effective = cap == 0 ? DEFAULT_LAUNCH_BLOCKS : cap;
    CHECK( plan.launches.size() == ( expectCandidates + effective - 1 ) / effective );
    for ( size_t k = 0; k < plan.launches.size(); ++k ) {
        CHECK( plan.launches[k].first == k * effective );
        CHECK( plan.launches[k].count >= 1 && plan.launches[k].count <= effective );
    }

    /* fake launches: real blocks give their record, false positives a random one */
    const uint64_t base = 1000;   /* the window's output starts behind earlier windows' */
    ChainWalk walk( plan, data.data(), base );
    std::vector<uint8_t> result( base + 1, 0xEE );
    for ( uint32_t k = 0; k < plan.launches.size(); ++k ) {
        const Launch& l = plan.launches[k];
        std::vector<Record> records( l.count );
        std::vector<uint8_t> output;
        for ( uint32_t i = 0; i < l.count; ++i ) {
            const uint32_t c = l.first + i;
            const uint32_t b = plan.buffer[c];
            const uint64_t rel = plan.bits[c] - 8 * plan.start[b];
            Record r;
            const auto it = specs[b].blocks.find( rel );
            if ( it != specs[b].blocks.end() ) {
                r = { it->second.length, it->second.status == MI355X_BZ2_OK ? it->second.decoded : 0, 0, it->second.crc,
                      it->second.status };
            } else {
                r = { 80 + rng() % 5000, rng() % 3 == 0 ? 0 : rng() % 700, 0, (uint32_t)rng(),
                      rng() % 2 == 0 ? MI355X_BZ2_OK : MI355X_BZ2_ERR_INVALID_CODE };
                if ( r.status != MI355X_BZ2_OK ) r.decodedSize = 0;
            }
            r.dataOffset = output.size();
            for ( uint64_t j = 0; j < r.decodedSize; ++j ) output.push_back( decodedByte( b, rel, j ) );
            records[i] = r;
        }
        const auto pieces = walk.advance( k, records.data() );
        for ( const auto& p : pieces ) {
            CHECK( p.src + p.size <= output.size() );
            if ( p.src + p.size > output.size() ) continue;
            /* pieces of one launch never overlap in the result */
            for ( const auto& q : pieces ) {
                if ( &q != &p ) CHECK( p.dst + p.size <= q.dst || q.dst + q.size <= p.dst );
            }
            if ( result.size() < p.dst + p.size ) result.resize( p.dst + p.size, 0xEE );
            std::memcpy( result.data() + p.dst, output.data() + p.src, p.size );
        }
    }
    const auto& got = walk.finish();
    uint64_t at = base;
    for ( uint32_t b = 0; b < n; ++b ) {
        /* the reader's rule for a damaged first magic of a stream (Spec::endsOkAt) */
        bool endsOk = specs[b].endsOkAt != UINT64_MAX;
        for ( const auto m : scan( specs[b].data.bytes ) ) endsOk = endsOk && m < specs[b].endsOkAt;
        const BufferResult& w = endsOk ? specs[b].okWant : specs[b].want;
        const auto& wantPieces = endsOk ? specs[b].okPieces : specs[b].pieces;
        const BufferResult& g = got[b];
        CHECK( g.status == w.status );
        CHECK( g.errorOffsetBits == w.errorOffsetBits );
        CHECK( g.outputOffset == at );
        CHECK( g.decodedSize == w.decodedSize );
        if ( w.status == MI355X_BZ2_OK ) {
            CHECK( g.blocks == w.blocks );
            CHECK( g.streams == w.streams );
            CHECK( g.trailingGarbage == w.trailingGarbage );
            uint64_t o = g.outputOffset;
            for ( const auto& [bits, size] : wantPieces ) {
                for ( uint64_t j = 0; j < size; ++j, ++o ) {
                    if ( o >= result.size() || result[o] != decodedByte( b, bits, j ) ) {
                        CHECK( !"decoded byte in place" );
                        j = size;
                        break;
                    }
                }
            }
        }
        at += g.decodedSize;
    }
    CHECK( walk.end() == at );
}

Spec
valid( std::mt19937_64& rng, int streams, int blocksPerStream, bool fake = false )
{
    Builder B( rng );
    for ( int s = 0; s < streams; ++s ) {
        B.header();
        for ( int k = 0; k < blocksPerStream; ++k ) B.block( 200 + rng() % 3000, 1 + rng() % 900, MI355X_BZ2_OK, fake && k == 0 );
        B.eos();
    }
    return B.s;
}
}  // namespace

int
main()
{
    std::mt19937_64 rng( 12345 );

    /* windows at and around the budget, cut only between buffers; an oversized buffer alone */
    {
        currentCase = "windows";
        const uint64_t sizes[] = { 40, 60, 1, 99, 100, 0, 250, 50, 50 };
        const auto w = planWindows( sizes, 9, 100 );
        CHECK( w.size() == 5 );
        if ( w.size() == 5 ) {
            CHECK( w[0].first == 0 && w[0].count == 2 && w[0].bytes == 100 );   /* exactly the budget */
            CHECK( w[1].first == 2 && w[1].count == 2 && w[1].bytes == 100 );
            CHECK( w[2].first == 4 && w[2].count == 2 && w[2].bytes == 100 );   /* a 0-byte buffer rides along */
            CHECK( w[3].first == 6 && w[3].count == 1 && w[3].bytes == 250 );   /* larger than the budget: alone */
            CHECK( w[4].first == 7 && w[4].count == 2 && w[4].bytes == 100 );
        }
        const uint64_t one[] = { 101 };
        CHECK( planWindows( one, 1, 100 ).size() == 1 );
        CHECK( planWindows( one, 0, 100 ).empty() );
        const uint64_t zeros[] = { 0, 0, 0 };
        const auto z = planWindows( zeros, 3, 100 );
        CHECK( z.size() == 1 && z[0].count == 3 && z[0].bytes == 0 );
    }

    /* a match straddling two buffers: the first buffer ends with the first half of a block magic */
    {
        std::vector<Spec> specs;
        specs.push_back( valid( rng, 1, 2 ) );
        Builder B( rng );
        B.header();
        B.block( 500, 100 );
        B.eos();
        B.s.data.put( MI355X_BZ2_MAGIC_BLOCK >> 24, 24 );   /* 3 bytes of garbage: the magic's first half */
        B.s.want.trailingGarbage = true;
        specs.push_back( B.s );
        Builder C( rng );
        C.s.data.put( MI355X_BZ2_MAGIC_BLOCK & 0xFFFFFF, 24 );   /* the other half: no stream header */
        C.fail( MI355X_BZ2_ERR_STREAM_HEADER, 0 );
        specs.push_back( C.s );
        specs.push_back( valid( rng, 1, 1 ) );
        for ( uint32_t cap : { 1u, 2u, 7u, 512u } ) runCase( "straddle", specs, cap, rng );
    }

    /* multi-stream chains, trailing garbage, a false positive inside a block, launch caps with buffers spanning launches */
    {
        std::vector<Spec> specs;
        specs.push_back( valid( rng, 3, 4 ) );
        specs.push_back( valid( rng, 1, 9, /* fake */ true ) );
        Builder G( rng );
        G.header();
        G.block( 900, 50 );
        G.block( 1700, 0 );   /* a block that decodes to nothing */
        G.eos();
        G.garbage( 4096 );
        specs.push_back( G.s );
        Builder E( rng );   /* bz2.compress( b"" ): a header and an end-of-stream block */
        E.header();
        E.eos();
        specs.push_back( E.s );
        specs.push_back( valid( rng, 2, 1 ) );
        for ( uint32_t cap : { 1u, 2u, 7u, 512u, 0u } ) runCase( "chains", specs, cap, rng );
    }

    /* failures: a damaged magic (not a candidate), a stream-CRC mismatch, a failed block inside a multi-block buffer, an
     * empty buffer, a header only, a cut inside an end-of-stream block, a bad stream header; neighbours unaffected */
    {
        std::vector<Spec> specs;
        specs.push_back( valid( rng, 1, 3 ) );
        Builder M( rng );
        M.header();
        M.block( 700, 10 );
        M.block( 800, 20, MI355X_BZ2_OK, false, /* damaged magic */ true );
        M.block( 900, 30 );
        M.eos();
        specs.push_back( M.s );
        specs.push_back( valid( rng, 1, 2 ) );
        Builder S( rng );
        S.header();
        S.block( 600, 40 );
        S.block( 600, 40 );
        S.eos( /* wrong CRC */ true );
        specs.push_back( S.s );
        Builder F( rng );
        F.header();
        F.block( 1000, 300 );
        F.block( 1000, 300, MI355X_BZ2_ERR_CRC );
        F.block( 1000, 300 );
        F.eos();
        specs.push_back( F.s );
        Builder Z( rng );   /* 0 bytes: 0 bytes out */
        specs.push_back( Z.s );
        Builder J( rng );   /* junk without a stream header */
        J.garbage( 300 );
        J.s.want.trailingGarbage = false;
        J.fail( MI355X_BZ2_ERR_STREAM_HEADER, 0 );
        specs.push_back( J.s );
        Builder H( rng );   /* "BZh9" alone: no block behind the header, as the reader sees it */
        H.header();
        specs.push_back( H.s );
        Builder T( rng );   /* cut 4 bytes into the end-of-stream block */
        T.header();
        T.block( 1234, 77 );
        const uint64_t eosAt = T.s.data.n;
        T.eos();
        T.s.data.bytes.resize( ( eosAt + 7 ) / 8 + 4 );
        T.s.data.n = 8 * T.s.data.bytes.size();
        T.fail( MI355X_BZ2_ERR_EOF, eosAt );
        T.s.want.streams = 0;
        specs.push_back( T.s );
        Builder X( rng );   /* a bad stream header */
        X.header( 'x' );
        X.block( 500, 5 );
        X.eos();
        X.failed = false;
        X.fail( MI355X_BZ2_ERR_STREAM_HEADER, 0 );
        specs.push_back( X.s );
        specs.push_back( valid( rng, 1, 5 ) );
        for ( uint32_t cap : { 1u, 2u, 7u, 512u } ) runCase( "failures", specs, cap, rng );
    }

    /* a damaged first magic of a stream: ERR_BAD_MAGIC if a block magic follows it in the buffer, else the buffer ends
     * there without error (what the reader's scan-driven walk does) */
    {
        std::vector<Spec> specs;
        Builder A( rng );   /* a real block follows: ERR_BAD_MAGIC */
        A.header();
        A.block( 700, 10, MI355X_BZ2_OK, false, /* damaged magic */ true );
        A.block( 900, 30 );
        A.eos();
        specs.push_back( A.s );
        Builder B( rng );   /* nothing follows: OK, 0 bytes */
        B.header();
        B.block( 700, 10, MI355X_BZ2_OK, false, true );
        B.eos();
        specs.push_back( B.s );
        Builder C( rng );   /* the second stream's first magic, nothing behind it: OK with the first stream's bytes */
        C.header();
        C.block( 800, 40 );
        C.block( 600, 20 );
        C.eos();
        C.header();
        C.block( 500, 10, MI355X_BZ2_OK, false, true );
        C.eos();
        specs.push_back( C.s );
        Builder D( rng );   /* a fake magic inside a later block's payload is a candidate too: ERR_BAD_MAGIC */
        D.header();
        D.block( 500, 10, MI355X_BZ2_OK, false, true );
        D.s.data.put( 0, 7 );
        D.s.data.put( MI355X_BZ2_MAGIC_BLOCK, 48 );
        D.s.data.pad();
        specs.push_back( D.s );
        specs.push_back( valid( rng, 1, 2 ) );
        for ( uint32_t cap : { 1u, 2u, 512u } ) runCase( "damaged first magic", specs, cap, rng );
        currentCase = "damaged first magic: expectations";
        bool endsOk[4];
        for ( int i = 0; i < 4; ++i ) {
            endsOk[i] = specs[i].endsOkAt != UINT64_MAX;
            for ( const auto m : scan( specs[i].data.bytes ) ) endsOk[i] = endsOk[i] && m < specs[i].endsOkAt;
        }
        CHECK( !endsOk[0] && endsOk[1] && endsOk[2] && !endsOk[3] );
        CHECK( specs[2].okWant.streams == 1 && specs[2].okWant.blocks == 2 && specs[2].okWant.decodedSize == 60 );
    }

    /* seeded mixtures, under several seeds */
    for ( const uint64_t seed : { 12345ull, 1ull, 2ull, 3ull, 5ull, 6ull, 7ull, 8ull, 2024ull } ) {
        rng.seed( seed );
        for ( int round = 0; round < 30; ++round ) {
            std::vector<Spec> specs;
            const int n = 1 + (int)( rng() % 12 );
            for ( int i = 0; i < n; ++i ) {
                Builder B( rng );
                const int streams = 1 + (int)( rng() % 3 );
                for ( int s = 0; s < streams; ++s ) {
                    B.header();
                    const int blocks = (int)( rng() % 5 );
                    for ( int k = 0; k < blocks; ++k ) {
                        const int32_t status = rng() % 15 == 0 ? MI355X_BZ2_ERR_CRC : MI355X_BZ2_OK;
                        B.block( 100 + rng() % 4000, rng() % 2000, status, rng() % 4 == 0, rng() % 30 == 0 );
                    }
                    B.eos( rng() % 20 == 0 );
                }
                if ( rng() % 6 == 0 ) B.garbage( 1 + rng() % 64 );
                specs.push_back( B.s );
            }
            const uint32_t caps[] = { 1, 2, 7, 512 };
            runCase( "seeded", specs, caps[round % 4], rng );
        }
    }

    if ( failures != 0 ) {
        std::printf( "%d failures\n", failures );
        return 1;
    }
    std::printf( "buffers ok\n" );
    return 0;
}
