/**
 * ibzip2-mi355x -- command line front end over the C ABI (include/mi355x_bz2.h).
 *
 * Mirrors the options and the behaviour of the reference tool `ibzip2` (src/tools/ibzip2.cpp:172-480): -c -d -f -i -o
 * -k -t -p -P -h -q -v -V -l -L --buffer-size, the same rules for the output file name, for refusing to overwrite,
 * for where the offset lists go (file / stdout / stderr) and the same two text formats:
 *   -l : one compressed bit offset per line                                   (dumpOffsets, ibzip2.cpp:68-80)
 *   -L : "<compressed bit offset>,<decoded byte offset>" per line             (dumpOffsets, ibzip2.cpp:83-93)
 * The reference parses its command line with cxxopts (an un-vendored submodule); this parser is our own.
 *
 * Differences: -P is the number of blocks kept in flight per GPU batch and defaults to 0 = automatic (512): there is no
 * serial CPU decoder behind -P 1, which would mean one block per GPU launch here.  What the reference's serial decoder
 * checks and its parallel one does not -- the combined CRC of every stream -- is checked with -t (and with -P 1).
 * Standard input is read completely into memory first (the GPU decodes from a resident copy anyway).
 */
#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/mi355x_bz2.h"

namespace
{
struct Options
{
    bool toStdout{ false }, decompress{ false }, force{ false }, keep{ false }, test{ false }, help{ false };
    bool quiet{ false }, version{ false };
    int verbose{ 0 };
    bool listCompressed{ false }, listOffsets{ false }, countLines{ false }, countMatches{ false }, grep{ false }, lineNumber{ false };
    bool grepFile{ false }, countMatchesFile{ false }, ignoreCase{ false }, grepRegex{ false };
    bool lineHashes{ false }, countDistinctLines{ false }, hasSeed{ false };
    uint64_t seed{ 0 };
    bool cutField{ false }, hasFieldDelimiter{ false }, countByField{ false };
    std::vector<uint32_t> cutFields;            /* --cut-fields: not empty iff given */
    bool sumByField{ false };
    bool whereField{ false }, whereEquals{ false }, whereInFile{ false }, whereBetween{ false }, invertMatch{ false };
    bool whereMatches{ false };
    bool hasLow{ false }, hasHigh{ false };
    int64_t low{ 0 }, high{ 0 };
    std::string equals, valueFile, matches;
    unsigned field{ 0 }, valueField{ 0 };
    uint8_t fieldDelimiter{ '\t' };
    bool hasFieldQuote{ false };                /* --field-quote */
    uint8_t fieldQuote{ '"' };
    std::string input, output, listCompressedPath, listOffsetsPath, pattern, patternFile, regex;
    bool hasOutput{ false };
    unsigned finderParallelism{ 1 }, decoderParallelism{ 0 }, bufferSize{ 0 };
    int device{ -1 };
};

void
printHelp()
{
    std::cout <<
        "A bzip2 decompressor tool based on the MI355X block decoder (drop-in for ibzip2)\n"
        "Usage:\n"
        "  ibzip2-mi355x [OPTION...] [input file]\n\n"
        " Decompression options:\n"
        "  -c, --stdout                  Output to standard output. This is the default, when reading from standard input.\n"
        "  -d, --decompress              Force decompression. Only for compatibility. No compression supported anyways.\n"
        "  -f, --force                   Force overwriting existing output files.\n"
        "  -i, --input arg               Input file. If none is given, data is read from standard input.\n"
        "  -o, --output arg              Output file. If none is given, use the input file name with '.bz2' stripped or\n"
        "                                '<input file>.out'.\n"
        "  -k, --keep                    Keep (do not delete) input file. Only for compatibility.\n"
        "  -t, --test                    Test compressed file integrity.\n"
        "  -p, --block-finder-parallelism arg\n"
        "                                Threads of the host block finder (0 = automatic). (default: 1)\n"
        "  -P, --decoder-parallelism arg Blocks kept in flight per GPU batch (0 = automatic). (default: 0; the\n"
        "                                reference defaults to 1 = its serial CPU decoder, which does not exist here)\n"
        "      --device arg              GPU to use (default: current device)\n\n"
        " Output options:\n"
        "  -h, --help                    Print this help message.\n"
        "  -q, --quiet                   Suppress noncritical error messages.\n"
        "  -v, --verbose                 Be verbose. A second -v (or shorthand -vv) gives even more verbosity.\n"
        "  -V, --version                 Display software version.\n"
        "  -l, --list-compressed-offsets [arg]\n"
        "                                List only the bzip2 block offsets given in bits one per line to the specified\n"
        "                                output file. If no file is given, it will print to stdout or to stderr if the\n"
        "                                decoded data is already written to stdout.\n"
        "  -L, --list-offsets [arg]      List bzip2 block offsets in bits and also the corresponding offsets in the\n"
        "                                decoded data at the beginning of each block in bytes as comma separated pairs\n"
        "                                per line '<encoded bits>,<decoded bytes>'.\n"
        "      --count-lines             Count the newline characters of the decoded data on the GPU (nothing is\n"
        "                                decompressed to the host), print the number and exit.\n"
        "      --count-matches arg       Count the occurrences of the given string (1 to 256 bytes; occurrences that\n"
        "                                overlap each other all count) in the decoded data on the GPU, print the\n"
        "                                number and exit.\n"
        "      --grep arg                Print the lines of the decoded data that contain the given string (1 to 256\n"
        "                                bytes, taken literally as by grep -F) in file order, each once, and exit.\n"
        "                                Matches and lines are found on the GPU; only the matching lines are copied\n"
        "                                to the host. The exit status is 0 whether or not a line matched: 1 means\n"
        "                                error here.\n"
        "      --grep-file arg           As --grep, for every string of a set at once (grep -F -f): the strings are the\n"
        "                                lines of the given file (1 to 1024 of them, 1 to 256 bytes each, at most 16384\n"
        "                                bytes in total; a final empty line is ignored, any other empty line refused).\n"
        "                                A line that contains several of them is printed once. The data is decoded\n"
        "                                once for the search whatever the number of strings.\n"
        "      --grep-regex arg          As --grep, for a regular expression (bzgrep PATTERN): print the lines whose\n"
        "                                content matches it. The syntax is a subset of Python's bytes re syntax with\n"
        "                                re.DOTALL: literals, . [...] [^...] \\d \\w \\s \\D \\W \\S \\n \\t \\xHH, ( ) (?: ) |,\n"
        "                                * + ? {m} {m,} {m,n} {,n}, ^ and $. Back-references, look-around, lazy\n"
        "                                quantifiers, \\b and patterns that need more than 64 DFA states are refused.\n"
        "                                --line-number and --ignore-case apply as for --grep.\n"
        "      --line-hashes             Print one hash per line of the decoded data, 16 lower-case hexadecimal digits\n"
        "                                each: h = (h * x + byte + 1) mod (2^61 - 1) over the line without its newline,\n"
        "                                x chosen by --seed. Equal lines have equal hashes; the data stays on the GPU.\n"
        "      --count-distinct-lines    Print the number of distinct line hashes (sort -u | wc -l). Distinct lines\n"
        "                                have distinct hashes with overwhelming probability, not with certainty: run\n"
        "                                again with another --seed for an independent check.\n"
        "      --seed arg                With --line-hashes or --count-distinct-lines: the 64-bit seed of the hash's\n"
        "                                base. (default: 0)\n"
        "      --cut-field arg           Print field N (counted from 0, at most 1023) of every line of the decoded\n"
        "                                data, one per line, and an empty line where a line has no such field (cut -f,\n"
        "                                awk -F): a line is split at every --field-delimiter byte; there is no quoting\n"
        "                                and no escaping, this is not a CSV parser. The fields are found on the GPU and\n"
        "                                only their bytes are copied to the host.\n"
        "      --cut-fields arg          Given N[,N...] (1 to 16 field numbers as for --cut-field, in any order, one may\n"
        "                                repeat): print those fields of every line in the order given, joined by the\n"
        "                                --field-delimiter byte, one line per line (cut -f1,4,6); a field a line does\n"
        "                                not have prints as empty. The data is decoded once, whatever the number of\n"
        "                                fields, and the GPU packs each field's bytes. This is not a CSV parser.\n"
        "      --field-delimiter arg     With --cut-field: the byte between fields, as itself (',') or as \\t, \\0 or\n"
        "                                \\xHH; not the newline. (default: \\t)\n"
        "      --field-quote arg         With --cut-field or --cut-fields: the byte that quotes fields, given as for\n"
        "                                --field-delimiter; not the newline or the delimiter. A delimiter between two\n"
        "                                quote bytes does not split the line, and a field enclosed in a pair of quote\n"
        "                                bytes prints without the pair; doubled quotes inside stay doubled, and a\n"
        "                                newline always ends the line. (default: no quoting)\n"
        "      --count-by-field arg      Print how often every value of field N (as for --cut-field) occurs, one line\n"
        "                                'count<TAB>value' per distinct value, the most frequent first and values of\n"
        "                                equal count in the order of their first occurrence (cut -f | sort | uniq -c |\n"
        "                                sort -rn); lines without the field are not counted. The lines are grouped on\n"
        "                                the GPU by a hash of the field (--seed chooses its base): distinct values have\n"
        "                                distinct hashes with overwhelming probability, not with certainty. Only the\n"
        "                                values' bytes are copied to the host. --field-delimiter applies; this is not a\n"
        "                                CSV parser.\n"
        "      --sum-by-field arg        Given KEY,VALUE (two field numbers as for --cut-field): print one line\n"
        "                                'sum<TAB>numbers<TAB>key' per distinct value of field KEY, in the order of their\n"
        "                                first occurrence: the exact sum of field VALUE over the lines with that key, and\n"
        "                                how many of them hold a number there (awk '{s[$1]+=$3}'). A number is\n"
        "                                [+-]?[0-9]{1,18} from end to end, not awk's strtod: anything else adds nothing.\n"
        "                                Lines without field KEY are in no group. The data is decoded once; keys\n"
        "                                (grouped by a hash, --seed chooses its base) and numbers are found and summed\n"
        "                                on the GPU. --field-delimiter applies; this is not a CSV parser.\n"
        "      --where-field arg         Given N (a field number as for --cut-field): print the lines whose field N\n"
        "                                satisfies ONE of --equals, --in-file or --between, whole and in file order, as\n"
        "                                --grep prints them (awk -F'\\t' '$3 == \"GET\"'). The field must be equal byte for\n"
        "                                byte; a line without field N is not selected. The data is decoded once and the\n"
        "                                rows are chosen on the GPU (a hash, whose base --seed chooses, only filters in\n"
        "                                front of the comparison of the bytes); the selected lines come in a second\n"
        "                                pass. The exit status is 0 whether or not a line was selected.\n"
        "                                --field-delimiter and --line-number apply; this is not a CSV parser.\n"
        "      --equals arg              With --where-field: the one value the field must be equal to; may be empty.\n"
        "      --in-file arg             With --where-field: the field must be equal to one line of the given file (a\n"
        "                                semi-join): 1 to 1024 values of at most 256 bytes, 16384 bytes in total, read\n"
        "                                as --grep-file reads its file.\n"
        "      --between arg             With --where-field: given LO,HI (either side may be empty: open), the field\n"
        "                                must be a number n with LO <= n <= HI (awk '$5 >= 500 && $5 <= 599'). A\n"
        "                                number is [+-]?[0-9]{1,18} from end to end, not awk's strtod.\n"
        "      --matches arg             With --where-field: the field must match the given regular expression, the\n"
        "                                fourth alternative beside --equals, --in-file and --between (awk -F'\\t'\n"
        "                                '$7 ~ /^\\/api\\//'). The syntax is --grep-regex's; the field is to the pattern\n"
        "                                what the line is to --grep-regex: ^ and $ anchor to the field's ends, and a\n"
        "                                line without field N does not match. --ignore-case applies, within\n"
        "                                --where-field with --matches only.\n"
        "      --invert-match            With --where-field: print the lines that are NOT selected (grep -v), those\n"
        "                                without field N included.\n"
        "      --count-matches-file arg  As --count-matches, for every line of the given file at once: one count per\n"
        "                                line, in the file's order.\n"
        "      --line-number             With --grep or --grep-file: prefix each line with its 1-based line number\n"
        "                                and ':'.\n"
        "      --ignore-case             With --grep, --grep-file, --count-matches or --count-matches-file: ignore the\n"
        "                                case of the ASCII letters A-Z and a-z, in the strings and in the data, as\n"
        "                                LC_ALL=C grep -i does. Every other byte must be equal. There is no short\n"
        "                                form: -i is --input.\n\n"
        " Advanced options:\n"
        "      --buffer-size arg         Controls the output buffer size. By default, the decoded data is written in\n"
        "                                one pass per block. (default: 0)\n\n"
        "Examples:\n\n"
        "Decompress a file:\n  ibzip2-mi355x -d file.bz2\n\n"
        "Decompress a file with 256 blocks per GPU batch:\n  ibzip2-mi355x -d -P 256 file.bz2\n\n"
        "Find and list the bzip2 block offsets to be used for another tool:\n"
        "  ibzip2-mi355x -l blockoffsets.dat -- file.bz2\n\n"
        "List block offsets in both the compressed as well as the decompressed data:\n"
        "  ibzip2-mi355x -L blockoffsets.dat file.bz2 > /dev/null\n\n"
        "Count the lines of a compressed file:\n"
        "  ibzip2-mi355x --count-lines file.bz2\n\n"
        "Count the occurrences of a string in a compressed file:\n"
        "  ibzip2-mi355x --count-matches ERROR file.bz2\n\n"
        "Print the lines of a compressed file that contain a string, with their numbers:\n"
        "  ibzip2-mi355x --grep ERROR --line-number file.bz2\n\n"
        "Print the lines that contain any of the strings listed in a file:\n"
        "  ibzip2-mi355x --grep-file codes.txt file.bz2\n\n"
        "Print the lines that contain a string in any case (error, Error, ERROR):\n"
        "  ibzip2-mi355x --grep error --ignore-case file.bz2\n\n"
        "Count the distinct lines of a file:\n"
        "  ibzip2-mi355x --count-distinct-lines file.bz2\n\n"
        "Print the third column of a tab-separated file:\n"
        "  ibzip2-mi355x --cut-field 2 file.tsv.bz2\n\n"
        "Print the first, fourth and sixth column of a tab-separated file:\n"
        "  ibzip2-mi355x --cut-fields 0,3,5 file.tsv.bz2\n\n"
        "Print how often each value of the third column occurs, the most frequent first:\n"
        "  ibzip2-mi355x --count-by-field 2 file.tsv.bz2\n\n"
        "Sum the third column per value of the first:\n"
        "  ibzip2-mi355x --sum-by-field 0,2 file.tsv.bz2\n\n"
        "Print the rows whose fifth column is a 5xx status, with their line numbers:\n"
        "  ibzip2-mi355x --where-field 4 --between 500,599 --line-number file.tsv.bz2\n\n"
        "Print the rows whose seventh column starts with /api/v and a digit:\n"
        "  ibzip2-mi355x --where-field 6 --matches '^/api/v[0-9]' file.tsv.bz2\n\n"
        "Print the lines that start with a date and report an error:\n"
        "  ibzip2-mi355x --grep-regex '^[0-9]{4}-[0-9]{2}-[0-9]{2} .*(ERROR|FATAL)' file.bz2\n";
}

/** The patterns of --grep-file / --count-matches-file: the LF-separated lines of the file, concatenated, and their sizes.
 * A final empty line from a trailing LF is ignored; any other empty line, or a file that cannot be read, is refused. */
bool
readPatternFile( const std::string& path, std::string& patterns, std::vector<uint32_t>& sizes )
{
    std::ifstream file( path, std::ios::binary );
    if ( !file ) {
        std::cerr << "Could not open the pattern file '" << path << "'\n";
        return false;
    }
    const std::string text( ( std::istreambuf_iterator<char>( file ) ), std::istreambuf_iterator<char>() );
    for ( size_t at = 0; at < text.size(); ) {
        const auto lf = text.find( '\n', at );
        const size_t stop = lf == std::string::npos ? text.size() : lf;
        if ( stop == at ) {
            std::cerr << "The pattern file '" << path << "' holds an empty line (line " << sizes.size() + 1 << ")\n";
            return false;
        }
        patterns.append( text, at, stop - at );
        sizes.push_back( (uint32_t)std::min<size_t>( stop - at, 0xFFFFFFFFu ) );
        at = stop + 1;
    }
    return true;
}

bool
fileExists( const std::string& path )
{
    struct stat st{};
    return ::stat( path.c_str(), &st ) == 0;
}

bool
endsWithNoCase( const std::string& s, const std::string& suffix )
{
    if ( s.size() < suffix.size() ) return false;
    for ( size_t i = 0; i < suffix.size(); ++i ) {
        if ( std::tolower( (unsigned char)s[s.size() - suffix.size() + i] ) != std::tolower( (unsigned char)suffix[i] ) ) return false;
    }
    return true;
}

bool
parseUnsigned( const char* text, unsigned& value )
{
    if ( text == nullptr || *text == '\0' ) return false;
    char* end = nullptr;
    errno = 0;
    const unsigned long v = std::strtoul( text, &end, 10 );
    if ( errno != 0 || *end != '\0' || v > 0xFFFFFFFFul ) return false;
    value = (unsigned)v;
    return true;
}

/** A 64-bit seed: decimal digits only, no sign, no overflow. */
bool
parseSeed( const char* text, uint64_t& value )
{
    if ( text == nullptr || *text == '\0' ) return false;
    uint64_t v = 0;
    for ( const char* c = text; *c != '\0'; ++c ) {
        if ( *c < '0' || *c > '9' ) return false;
        const uint64_t digit = (uint64_t)( *c - '0' );
        if ( v > ( ~uint64_t( 0 ) - digit ) / 10 ) return false;
        v = v * 10 + digit;
    }
    value = v;
    return true;
}

/** One byte for --field-delimiter: the argument itself if it is one byte, or \\t, \\0, \\xHH. */
bool
parseByte( const std::string& text, uint8_t& value )
{
    const auto hex = [] ( char c ) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
    if ( text.size() == 1 ) value = (uint8_t)text[0];
    else if ( text == "\\t" ) value = '\t';
    else if ( text == "\\0" ) value = 0;
    else if ( text.size() == 4 && text[0] == '\\' && text[1] == 'x' && hex( text[2] ) >= 0 && hex( text[3] ) >= 0 ) {
        value = (uint8_t)( hex( text[2] ) * 16 + hex( text[3] ) );
    } else return false;
    return true;
}

/** Returns 0 on success.  An option with an optional value (-l, -L) takes the next argument unless that starts with '-'
 * or is the last argument while no input has been seen (then it is the positional input file, the ambiguity the
 * reference warns about, ibzip2.cpp:175-178, resolved the way its examples are written: "-l file -- input"). */
int
parseArguments( int argc, char** argv, Options& o )
{
    std::vector<std::string> positional;
    bool onlyPositional = false;
    const auto optionalValue = [&] ( int& i, std::string& path ) {
        if ( i + 1 < argc && argv[i + 1][0] != '-' && !( i + 2 == argc && o.input.empty() && positional.empty() ) ) {
            path = argv[++i];
        }
    };
    const auto requiredValue = [&] ( int& i, const std::string& name, std::string& out ) -> bool {
        if ( i + 1 >= argc ) {
            std::cerr << "Option '" << name << "' is missing an argument\n";
            return false;
        }
        out = argv[++i];
        return true;
    };
    for ( int i = 1; i < argc; ++i ) {
        const std::string a = argv[i];
        if ( onlyPositional || a.empty() || a[0] != '-' || a == "-" ) {
            positional.push_back( a );
            continue;
        }
        if ( a == "--" ) { onlyPositional = true; continue; }
        std::string value;
        if ( a.rfind( "--", 0 ) == 0 ) {
            std::string name = a.substr( 2 ), inlineValue;
            bool hasInline = false;
            const auto eq = name.find( '=' );
            if ( eq != std::string::npos ) {
                inlineValue = name.substr( eq + 1 );
                name = name.substr( 0, eq );
                hasInline = true;
            }
            const auto need = [&] ( std::string& out ) -> bool {
                if ( hasInline ) { out = inlineValue; return true; }
                return requiredValue( i, "--" + name, out );
            };
            if ( name == "stdout" ) o.toStdout = true;
            else if ( name == "decompress" ) o.decompress = true;
            else if ( name == "force" ) o.force = true;
            else if ( name == "keep" ) o.keep = true;
            else if ( name == "test" ) o.test = true;
            else if ( name == "help" ) o.help = true;
            else if ( name == "quiet" ) o.quiet = true;
            else if ( name == "verbose" ) ++o.verbose;
            else if ( name == "version" ) o.version = true;
            else if ( name == "input" ) { if ( !need( o.input ) ) return 1; }
            else if ( name == "output" ) { if ( !need( o.output ) ) return 1; o.hasOutput = true; }
            else if ( name == "count-lines" ) o.countLines = true;
            else if ( name == "count-matches" ) { if ( !need( o.pattern ) ) return 1; o.countMatches = true; }
            else if ( name == "grep" ) { if ( !need( o.pattern ) ) return 1; o.grep = true; }
            else if ( name == "grep-regex" ) { if ( !need( o.regex ) ) return 1; o.grepRegex = true; }
            else if ( name == "line-hashes" ) o.lineHashes = true;
            else if ( name == "count-distinct-lines" ) o.countDistinctLines = true;
            else if ( name == "seed" ) {
                if ( !need( value ) || !parseSeed( value.c_str(), o.seed ) ) { std::cerr << "Bad value for --seed\n"; return 1; }
                o.hasSeed = true;
            }
            else if ( name == "cut-field" ) {
                uint64_t field = 0;     /* digits only, as --seed */
                if ( !need( value ) || !parseSeed( value.c_str(), field ) || field > 1023 ) {
                    std::cerr << "Bad value for --cut-field\n";
                    return 1;
                }
                o.field = (unsigned)field;
                o.cutField = true;
            }
            else if ( name == "cut-fields" ) {
                /* N[,N...]: digits only, as --cut-field; no empty list, no empty entry, at most 16 */
                bool good = need( value ) && !value.empty();
                for ( size_t from = 0; good && from <= value.size(); ) {
                    const auto comma = std::min( value.find( ',', from ), value.size() );
                    uint64_t field = 0;
                    good = parseSeed( value.substr( from, comma - from ).c_str(), field ) && field <= 1023 && o.cutFields.size() < 16;
                    if ( good ) o.cutFields.push_back( (uint32_t)field );
                    from = comma + 1;
                }
                if ( !good ) {
                    std::cerr << "Bad value for --cut-fields\n";
                    return 1;
                }
            }
            else if ( name == "count-by-field" ) {
                uint64_t field = 0;     /* digits only, as --cut-field */
                if ( !need( value ) || !parseSeed( value.c_str(), field ) || field > 1023 ) {
                    std::cerr << "Bad value for --count-by-field\n";
                    return 1;
                }
                o.field = (unsigned)field;
                o.countByField = true;
            }
            else if ( name == "sum-by-field" ) {
                uint64_t key = 0, number = 0;     /* KEY,VALUE: digits only, as --cut-field */
                const bool given = need( value );
                const auto comma = value.find( ',' );
                if ( !given || comma == std::string::npos || !parseSeed( value.substr( 0, comma ).c_str(), key ) || key > 1023
                     || !parseSeed( value.substr( comma + 1 ).c_str(), number ) || number > 1023 ) {
                    std::cerr << "Bad value for --sum-by-field\n";
                    return 1;
                }
                o.field = (unsigned)key;
                o.valueField = (unsigned)number;
                o.sumByField = true;
            }
            else if ( name == "where-field" ) {
                uint64_t field = 0;     /* digits only, as --cut-field */
                if ( !need( value ) || !parseSeed( value.c_str(), field ) || field > 1023 ) {
                    std::cerr << "Bad value for --where-field\n";
                    return 1;
                }
                o.field = (unsigned)field;
                o.whereField = true;
            }
            else if ( name == "equals" ) { if ( !need( o.equals ) ) return 1; o.whereEquals = true; }
            else if ( name == "in-file" ) { if ( !need( o.valueFile ) ) return 1; o.whereInFile = true; }
            else if ( name == "between" ) {
                /* LO,HI: each side empty or [+-]?digits, at most 18 of them */
                const bool given = need( value );
                const auto comma = value.find( ',' );
                const auto bound = [] ( const std::string& text, bool& has, int64_t& number ) {
                    has = !text.empty();
                    if ( !has ) return true;
                    const size_t from = text[0] == '-' || text[0] == '+' ? 1 : 0;
                    uint64_t magnitude = 0;
                    if ( text.size() - from > 18 || !parseSeed( text.c_str() + from, magnitude ) ) return false;
                    number = text[0] == '-' ? -(int64_t)magnitude : (int64_t)magnitude;
                    return true;
                };
                if ( !given || comma == std::string::npos || !bound( value.substr( 0, comma ), o.hasLow, o.low )
                     || !bound( value.substr( comma + 1 ), o.hasHigh, o.high ) ) {
                    std::cerr << "Bad value for --between\n";
                    return 1;
                }
                o.whereBetween = true;
            }
            else if ( name == "matches" ) { if ( !need( o.matches ) ) return 1; o.whereMatches = true; }
            else if ( name == "invert-match" ) o.invertMatch = true;
            else if ( name == "field-delimiter" ) {
                if ( !need( value ) || !parseByte( value, o.fieldDelimiter ) || o.fieldDelimiter == '\n' ) {
                    std::cerr << "Bad value for --field-delimiter\n";
                    return 1;
                }
                o.hasFieldDelimiter = true;
            }
            else if ( name == "field-quote" ) {
                if ( !need( value ) || !parseByte( value, o.fieldQuote ) || o.fieldQuote == '\n' ) {
                    std::cerr << "Bad value for --field-quote\n";
                    return 1;
                }
                o.hasFieldQuote = true;
            }
            else if ( name == "grep-file" ) { if ( !need( o.patternFile ) ) return 1; o.grepFile = true; }
            else if ( name == "count-matches-file" ) { if ( !need( o.patternFile ) ) return 1; o.countMatchesFile = true; }
            else if ( name == "line-number" ) o.lineNumber = true;
            else if ( name == "ignore-case" ) o.ignoreCase = true;
            else if ( name == "list-compressed-offsets" ) {
                o.listCompressed = true;
                if ( hasInline ) o.listCompressedPath = inlineValue; else optionalValue( i, o.listCompressedPath );
            } else if ( name == "list-offsets" ) {
                o.listOffsets = true;
                if ( hasInline ) o.listOffsetsPath = inlineValue; else optionalValue( i, o.listOffsetsPath );
            } else if ( name == "block-finder-parallelism" ) {
                if ( !need( value ) || !parseUnsigned( value.c_str(), o.finderParallelism ) ) { std::cerr << "Bad value for --" << name << "\n"; return 1; }
            } else if ( name == "decoder-parallelism" ) {
                if ( !need( value ) || !parseUnsigned( value.c_str(), o.decoderParallelism ) ) { std::cerr << "Bad value for --" << name << "\n"; return 1; }
            } else if ( name == "buffer-size" ) {
                if ( !need( value ) || !parseUnsigned( value.c_str(), o.bufferSize ) ) { std::cerr << "Bad value for --" << name << "\n"; return 1; }
            } else if ( name == "device" ) {
                unsigned d = 0;
                if ( !need( value ) || !parseUnsigned( value.c_str(), d ) ) { std::cerr << "Bad value for --device\n"; return 1; }
                o.device = (int)d;
            } else {
                std::cerr << "Option '" << name << "' does not exist\n";
                return 1;
            }
            continue;
        }
        /* bundle of short options, e.g. -dvv or -P0 */
        for ( size_t k = 1; k < a.size(); ++k ) {
            const char c = a[k];
            const auto rest = [&] ( std::string& out ) -> bool {   /* value glued to the option or the next argument */
                if ( k + 1 < a.size() ) { out = a.substr( k + 1 ); k = a.size(); return true; }
                return requiredValue( i, std::string( "-" ) + c, out );
            };
            switch ( c ) {
            case 'c': o.toStdout = true; break;
            case 'd': o.decompress = true; break;
            case 'f': o.force = true; break;
            case 'k': o.keep = true; break;
            case 't': o.test = true; break;
            case 'h': o.help = true; break;
            case 'q': o.quiet = true; break;
            case 'v': ++o.verbose; break;
            case 'V': o.version = true; break;
            case 'i': if ( !rest( o.input ) ) return 1; break;
            case 'o': if ( !rest( o.output ) ) return 1; o.hasOutput = true; break;
            case 'p': if ( !rest( value ) || !parseUnsigned( value.c_str(), o.finderParallelism ) ) { std::cerr << "Bad value for -p\n"; return 1; } break;
            case 'P': if ( !rest( value ) || !parseUnsigned( value.c_str(), o.decoderParallelism ) ) { std::cerr << "Bad value for -P\n"; return 1; } break;
            case 'l':
                o.listCompressed = true;
                if ( k + 1 < a.size() ) { o.listCompressedPath = a.substr( k + 1 ); k = a.size(); } else optionalValue( i, o.listCompressedPath );
                break;
            case 'L':
                o.listOffsets = true;
                if ( k + 1 < a.size() ) { o.listOffsetsPath = a.substr( k + 1 ); k = a.size(); } else optionalValue( i, o.listOffsetsPath );
                break;
            default:
                std::cerr << "Option '" << c << "' does not exist\n";
                return 1;
            }
        }
    }
    if ( positional.size() + ( o.input.empty() ? 0 : 1 ) > 1 ) {
        std::cerr << "One or none bzip2 filename to decompress must be specified!\n";
        return 1;
    }
    if ( !positional.empty() ) o.input = positional.front();
    return 0;
}

bool
stdinHasInput()
{
    return !::isatty( STDIN_FILENO );
}

/** Whole input in memory: a mapping for files, a vector for standard input. */
struct Input
{
    const uint8_t* data{ nullptr };
    uint64_t size{ 0 };
    std::vector<uint8_t> owned;
    void* mapping{ nullptr };
    ~Input() { if ( mapping != nullptr ) ::munmap( mapping, size ); }

    bool
    open( const std::string& path )
    {
        if ( path.empty() ) {
            uint8_t buffer[1 << 16];
            for ( ;; ) {
                const ssize_t n = ::read( STDIN_FILENO, buffer, sizeof( buffer ) );
                if ( n < 0 && errno == EINTR ) continue;
                if ( n <= 0 ) break;
                owned.insert( owned.end(), buffer, buffer + n );
            }
            data = owned.data();
            size = owned.size();
            return true;
        }
        const int fd = ::open( path.c_str(), O_RDONLY );
        if ( fd < 0 ) return false;
        struct stat st{};
        if ( ::fstat( fd, &st ) != 0 ) { ::close( fd ); return false; }
        size = (uint64_t)st.st_size;
        if ( size > 0 ) {
            mapping = ::mmap( nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0 );
            if ( mapping == MAP_FAILED ) { mapping = nullptr; ::close( fd ); return false; }
            data = static_cast<const uint8_t*>( mapping );
        }
        ::close( fd );
        return true;
    }
};

constexpr uint64_t MAGIC_BLOCK = 0x314159265359ull;
constexpr uint64_t MAGIC_EOS = 0x177245385090ull;

/** checkOffsets, ibzip2.cpp:37-65: every listed offset must point at one of the two 48-bit magics. */
bool
checkOffsets( const Input& in, const std::vector<uint64_t>& offsets )
{
    for ( const auto offset : offsets ) {
        uint64_t magic = 0;
        bool inside = offset + 48 <= in.size * 8;
        for ( uint64_t b = offset; inside && b < offset + 48; ++b ) {
            magic = ( magic << 1 ) | ( ( in.data[b >> 3] >> ( 7 - ( b & 7 ) ) ) & 1u );
        }
        if ( !inside || ( magic != MAGIC_BLOCK && magic != MAGIC_EOS ) ) {
            std::cerr << "Magic bytes " << std::hex << magic << std::dec << " at offset " << ( offset / 8 ) << " B "
                      << ( offset % 8 ) << "b do not match bzip2 magic bytes!\n";
            return false;
        }
    }
    return true;
}

void
dumpOffsets( std::ostream& out, const std::vector<uint64_t>& offsets )
{
    if ( !out.good() ) return;
    for ( const auto offset : offsets ) out << offset << "\n";
}

void
dumpOffsets( std::ostream& out, const std::vector<uint64_t>& bits, const std::vector<uint64_t>& bytes )
{
    if ( !out.good() ) return;
    for ( size_t i = 0; i < bits.size(); ++i ) out << bits[i] << "," << bytes[i] << "\n";
}

/** findCompressedBlocks, ibzip2.cpp:96-139: both magics, sorted, no decoding (runs without a GPU). */
int
findCompressedBlocks( const Options& o )
{
    Input in;
    if ( !in.open( o.input ) ) {
        std::cerr << "Could not open '" << o.input << "'\n";
        return 1;
    }
    std::vector<uint64_t> offsets;
    for ( const auto magic : { MAGIC_BLOCK, MAGIC_EOS } ) {
        const uint64_t n = mi355x_bz2_find_magic( in.data, in.size, magic, nullptr, 0, o.finderParallelism );
        std::vector<uint64_t> found( n );
        mi355x_bz2_find_magic( in.data, in.size, magic, found.data(), n, o.finderParallelism );
        offsets.insert( offsets.end(), found.begin(), found.end() );
    }
    std::sort( offsets.begin(), offsets.end() );
    if ( o.test && !checkOffsets( in, offsets ) ) return 1;
    if ( o.listCompressedPath.empty() ) {
        dumpOffsets( std::cout, offsets );
    } else {
        std::ofstream file( o.listCompressedPath );
        dumpOffsets( file, offsets );
    }
    if ( o.verbose > 0 ) std::cout << "Found " << offsets.size() << " blocks\n";
    return 0;
}
}  // namespace

int
main( int argc, char** argv )
{
    /* the reader drives two decoder contexts with four HIP streams each: give every stream its own hardware queue
     * (read by the HIP runtime when it starts; an existing setting wins) */
    ::setenv( "GPU_MAX_HW_QUEUES", "16", 0 );
    Options o;
    if ( parseArguments( argc, argv, o ) != 0 ) return 1;

    if ( o.help ) {
        printHelp();
        return 0;
    }
    if ( o.grep && o.countMatches ) {
        std::cerr << "Options '--grep' and '--count-matches' cannot be combined\n";
        return 1;
    }
    if ( (int)o.grep + (int)o.countMatches + (int)o.grepFile + (int)o.countMatchesFile > 1 ) {
        std::cerr << "Options '--grep', '--count-matches', '--grep-file' and '--count-matches-file' cannot be combined\n";
        return 1;
    }
    if ( o.grepRegex && ( o.grep || o.countMatches || o.grepFile || o.countMatchesFile ) ) {
        std::cerr << "Option '--grep-regex' cannot be combined with '--grep', '--count-matches', '--grep-file' or '--count-matches-file'\n";
        return 1;
    }
    if ( o.whereField && ( o.grep || o.countMatches || o.grepFile || o.countMatchesFile || o.grepRegex || o.countLines || o.lineHashes
                           || o.countDistinctLines || o.cutField || o.countByField || o.sumByField || !o.cutFields.empty() ) ) {
        std::cerr << "Option '--where-field' cannot be combined with '--count-lines', '--grep', '--grep-regex', '--count-matches', "
                     "'--grep-file', '--count-matches-file', '--line-hashes', '--count-distinct-lines', '--cut-field', '--cut-fields', "
                     "'--count-by-field' or '--sum-by-field'\n";
        return 1;
    }
    /* --matches is named only where it was given: the sentence below it is older than --matches, and its bytes are kept */
    if ( o.whereField && o.whereMatches && ( o.whereEquals || o.whereInFile || o.whereBetween ) ) {
        std::cerr << "Option '--where-field' needs exactly one of '--equals', '--in-file', '--between' and '--matches'\n";
        return 1;
    }
    if ( o.whereField && !o.whereMatches && (int)o.whereEquals + (int)o.whereInFile + (int)o.whereBetween != 1 ) {
        std::cerr << "Option '--where-field' needs exactly one of '--equals', '--in-file' and '--between'\n";
        return 1;
    }
    if ( !o.whereField && o.whereMatches ) {
        std::cerr << "Option '--matches' needs '--where-field'\n";
        return 1;
    }
    if ( !o.whereField && ( o.whereEquals || o.whereInFile || o.whereBetween || o.invertMatch ) ) {
        std::cerr << "Options '--equals', '--in-file', '--between' and '--invert-match' need '--where-field'\n";
        return 1;
    }
    if ( o.lineNumber && !o.grep && !o.grepFile && !o.grepRegex && !o.whereField ) {
        std::cerr << "Option '--line-number' needs '--grep' or '--grep-file'\n";
        return 1;
    }
    /* also accepted with --grep-regex and with --where-field --matches; the sentence's bytes are kept as they were */
    if ( o.ignoreCase && !o.grep && !o.grepFile && !o.countMatches && !o.countMatchesFile && !o.grepRegex && !o.whereMatches ) {
        std::cerr << "Option '--ignore-case' needs '--grep', '--grep-file', '--count-matches' or '--count-matches-file'\n";
        return 1;
    }
    if ( o.lineHashes && o.countDistinctLines ) {
        std::cerr << "Options '--line-hashes' and '--count-distinct-lines' cannot be combined\n";
        return 1;
    }
    if ( ( o.lineHashes || o.countDistinctLines )
         && ( o.grep || o.countMatches || o.grepFile || o.countMatchesFile || o.grepRegex || o.countLines ) ) {
        std::cerr << "Options '--line-hashes' and '--count-distinct-lines' cannot be combined with '--count-lines', '--grep', "
                     "'--grep-regex', '--count-matches', '--grep-file' or '--count-matches-file'\n";
        return 1;
    }
    if ( !o.cutFields.empty() && ( o.grep || o.countMatches || o.grepFile || o.countMatchesFile || o.grepRegex || o.countLines || o.lineHashes
                                   || o.countDistinctLines || o.cutField || o.countByField || o.sumByField ) ) {
        std::cerr << "Option '--cut-fields' cannot be combined with '--count-lines', '--grep', '--grep-regex', '--count-matches', "
                     "'--grep-file', '--count-matches-file', '--line-hashes', '--count-distinct-lines', '--cut-field', "
                     "'--count-by-field' or '--sum-by-field'\n";
        return 1;
    }
    if ( o.sumByField && ( o.grep || o.countMatches || o.grepFile || o.countMatchesFile || o.grepRegex || o.countLines || o.lineHashes
                           || o.countDistinctLines || o.cutField || o.countByField ) ) {
        std::cerr << "Option '--sum-by-field' cannot be combined with '--count-lines', '--grep', '--grep-regex', '--count-matches', "
                     "'--grep-file', '--count-matches-file', '--line-hashes', '--count-distinct-lines', '--cut-field' or "
                     "'--count-by-field'\n";
        return 1;
    }
    if ( o.countByField && ( o.grep || o.countMatches || o.grepFile || o.countMatchesFile || o.grepRegex || o.countLines || o.lineHashes
                             || o.countDistinctLines || o.cutField ) ) {
        std::cerr << "Option '--count-by-field' cannot be combined with '--count-lines', '--grep', '--grep-regex', '--count-matches', "
                     "'--grep-file', '--count-matches-file', '--line-hashes', '--count-distinct-lines' or '--cut-field'\n";
        return 1;
    }
    if ( o.hasSeed && !o.lineHashes && !o.countDistinctLines && !o.countByField && !o.sumByField && !o.whereField ) {
        std::cerr << "Option '--seed' needs '--line-hashes' or '--count-distinct-lines'\n";
        return 1;
    }
    if ( o.cutField && ( o.grep || o.countMatches || o.grepFile || o.countMatchesFile || o.grepRegex || o.countLines || o.lineHashes
                         || o.countDistinctLines ) ) {
        std::cerr << "Option '--cut-field' cannot be combined with '--count-lines', '--grep', '--grep-regex', '--count-matches', "
                     "'--grep-file', '--count-matches-file', '--line-hashes' or '--count-distinct-lines'\n";
        return 1;
    }
    if ( o.hasFieldDelimiter && !o.cutField && !o.countByField && !o.sumByField && o.cutFields.empty() && !o.whereField ) {
        std::cerr << "Option '--field-delimiter' needs '--cut-field'\n";
        return 1;
    }
    if ( o.hasFieldQuote && ( ( !o.cutField && o.cutFields.empty() ) || o.countByField || o.sumByField || o.whereField ) ) {
        std::cerr << "Option '--field-quote' needs '--cut-field' or '--cut-fields' and no other field option\n";
        return 1;
    }
    if ( o.hasFieldQuote && o.fieldQuote == o.fieldDelimiter ) {
        std::cerr << "Bad value for --field-quote\n";
        return 1;
    }
    const uint32_t searchFlags = o.ignoreCase ? MI355X_BZ2_SEARCH_IGNORE_CASE : 0u;
    if ( o.version ) {
        std::cout << "ibzip2-mi355x, CLI to the MI355X bzip2 block decoder (C ABI version " << mi355x_bz2_abi_version()
                  << "), option-compatible with ibzip2 of indexed-bzip2 1.7.0.\n";
        return 0;
    }
    if ( !stdinHasInput() && o.input.empty() ) {
        std::cerr << "Either stdin must have input, e.g., by piping to it, or an input file must be specified!\n";
        return 1;
    }

    /* an action of its own (rapidgzip --count-lines, src/tools/rapidgzip.cpp; ibzip2 has none): the number of newline
     * characters in the decoded data, from the reader's line index */
    if ( o.countLines ) {
        Input in;
        if ( !in.open( o.input ) ) {
            std::cerr << "Could not open '" << o.input << "'\n";
            return 1;
        }
        if ( mi355x_bz2_read_stream_header( in.data, in.size, 0 ) == 0 ) {
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( MI355X_BZ2_ERR_STREAM_HEADER ) << "\n";
            return 1;
        }
        mi355x_bz2_reader* reader = nullptr;
        int rc = mi355x_bz2_reader_open_memory( in.data, in.size, o.decoderParallelism, o.device, &reader );
        if ( rc != MI355X_BZ2_OK ) {
            std::cerr << "Could not open the bzip2 stream: " << mi355x_bz2_status_string( rc ) << "\n";
            return 1;
        }
        uint64_t count = 0;
        rc = mi355x_bz2_reader_line_offsets( reader, '\n', nullptr, nullptr, 0, &count );
        std::vector<uint64_t> bytes( count ), lines( count );
        if ( rc == MI355X_BZ2_OK ) rc = mi355x_bz2_reader_line_offsets( reader, '\n', bytes.data(), lines.data(), count, &count );
        if ( rc != MI355X_BZ2_OK || lines.empty() ) {
            const char* detail = mi355x_bz2_reader_last_error( reader );
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( rc );
            if ( detail != nullptr && detail[0] != '\0' ) std::cerr << " (" << detail << ")";
            std::cerr << "\n";
            mi355x_bz2_reader_close( reader );
            return 1;
        }
        mi355x_bz2_reader_close( reader );
        std::cout << lines.back() << "\n";
        return 0;
    }

    /* likewise actions of their own: one hash per line, from the reader's line_hashes, or the number of distinct ones,
     * from its distinct_lines */
    if ( o.lineHashes || o.countDistinctLines ) {
        Input in;
        if ( !in.open( o.input ) ) {
            std::cerr << "Could not open '" << o.input << "'\n";
            return 1;
        }
        if ( mi355x_bz2_read_stream_header( in.data, in.size, 0 ) == 0 ) {
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( MI355X_BZ2_ERR_STREAM_HEADER ) << "\n";
            return 1;
        }
        mi355x_bz2_reader* reader = nullptr;
        int rc = mi355x_bz2_reader_open_memory( in.data, in.size, o.decoderParallelism, o.device, &reader );
        if ( rc != MI355X_BZ2_OK ) {
            std::cerr << "Could not open the bzip2 stream: " << mi355x_bz2_status_string( rc ) << "\n";
            return 1;
        }
        uint64_t n = 0;
        std::vector<uint64_t> hashes;
        if ( o.countDistinctLines ) {
            rc = mi355x_bz2_reader_distinct_lines( reader, '\n', o.seed, 0, &n );
        } else {
            rc = mi355x_bz2_reader_line_hashes( reader, '\n', o.seed, 0, ~uint64_t( 0 ), 0, &n );
            hashes.resize( n );
            if ( rc == MI355X_BZ2_OK ) rc = mi355x_bz2_reader_take_line_hashes( reader, hashes.data(), n, 0 );
        }
        if ( rc != MI355X_BZ2_OK ) {
            const char* detail = mi355x_bz2_reader_last_error( reader );
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( rc );
            if ( detail != nullptr && detail[0] != '\0' ) std::cerr << " (" << detail << ")";
            std::cerr << "\n";
            mi355x_bz2_reader_close( reader );
            return 1;
        }
        mi355x_bz2_reader_close( reader );
        if ( o.countDistinctLines ) {
            std::cout << n << "\n";
            return 0;
        }
        std::string text( hashes.size() * 17, '\n' );
        for ( size_t i = 0; i < hashes.size(); ++i ) {
            for ( int digit = 0; digit < 16; ++digit ) text[i * 17 + digit] = "0123456789abcdef"[( hashes[i] >> ( 60 - 4 * digit ) ) & 15];
        }
        std::cout << text;
        return 0;
    }

    /* likewise an action of its own: one field of every line, from the reader's field_spans and read_ranges, in windows
     * of lines so that the memory is bounded whatever the file */
    if ( o.cutField ) {
        Input in;
        if ( !in.open( o.input ) ) {
            std::cerr << "Could not open '" << o.input << "'\n";
            return 1;
        }
        if ( mi355x_bz2_read_stream_header( in.data, in.size, 0 ) == 0 ) {
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( MI355X_BZ2_ERR_STREAM_HEADER ) << "\n";
            return 1;
        }
        mi355x_bz2_reader* reader = nullptr;
        int rc = mi355x_bz2_reader_open_memory( in.data, in.size, o.decoderParallelism, o.device, &reader );
        if ( rc != MI355X_BZ2_OK ) {
            std::cerr << "Could not open the bzip2 stream: " << mi355x_bz2_status_string( rc ) << "\n";
            return 1;
        }
        constexpr uint64_t WINDOW = uint64_t( 1 ) << 20;
        std::vector<uint64_t> starts, lengths, got;
        std::vector<int64_t> sizes;
        std::string bytes, text;
        for ( uint64_t first = 0; rc == MI355X_BZ2_OK; first += WINDOW ) {
            uint64_t n = 0;
            rc = o.hasFieldQuote ? mi355x_bz2_reader_field_spans_quoted( reader, '\n', o.fieldDelimiter, o.field, first, WINDOW, 0, &n, o.fieldQuote )
                                 : mi355x_bz2_reader_field_spans( reader, '\n', o.fieldDelimiter, o.field, first, WINDOW, 0, &n );
            if ( rc != MI355X_BZ2_OK || n == 0 ) break;
            starts.resize( n );
            sizes.resize( n );
            lengths.resize( n );
            got.resize( n );
            rc = mi355x_bz2_reader_take_field_spans( reader, starts.data(), sizes.data(), n, 0 );
            if ( rc != MI355X_BZ2_OK ) break;
            uint64_t total = 0;
            for ( uint64_t i = 0; i < n; ++i ) total += lengths[i] = sizes[i] > 0 ? (uint64_t)sizes[i] : 0;
            bytes.resize( total );
            rc = mi355x_bz2_reader_read_ranges( reader, starts.data(), lengths.data(), (uint32_t)n, bytes.data(), 0, got.data() );
            if ( rc != MI355X_BZ2_OK ) break;
            text.clear();
            text.reserve( total + n );
            uint64_t at = 0;
            for ( uint64_t i = 0; i < n; ++i ) {
                text.append( bytes, at, lengths[i] );
                text.push_back( '\n' );
                at += lengths[i];
            }
            std::cout << text;
            if ( n < WINDOW ) break;
        }
        if ( rc != MI355X_BZ2_OK ) {
            const char* detail = mi355x_bz2_reader_last_error( reader );
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( rc );
            if ( detail != nullptr && detail[0] != '\0' ) std::cerr << " (" << detail << ")";
            std::cerr << "\n";
            mi355x_bz2_reader_close( reader );
            return 1;
        }
        mi355x_bz2_reader_close( reader );
        return 0;
    }

    /* likewise an action of its own: several fields of every line from the reader's field_columns -- one decode, each
     * field packed on the GPU --, in windows of lines so that the memory is bounded whatever the file */
    if ( !o.cutFields.empty() ) {
        Input in;
        if ( !in.open( o.input ) ) {
            std::cerr << "Could not open '" << o.input << "'\n";
            return 1;
        }
        if ( mi355x_bz2_read_stream_header( in.data, in.size, 0 ) == 0 ) {
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( MI355X_BZ2_ERR_STREAM_HEADER ) << "\n";
            return 1;
        }
        mi355x_bz2_reader* reader = nullptr;
        int rc = mi355x_bz2_reader_open_memory( in.data, in.size, o.decoderParallelism, o.device, &reader );
        if ( rc != MI355X_BZ2_OK ) {
            std::cerr << "Could not open the bzip2 stream: " << mi355x_bz2_status_string( rc ) << "\n";
            return 1;
        }
        constexpr uint64_t WINDOW = uint64_t( 1 ) << 20;
        const size_t nFields = o.cutFields.size();
        std::vector<uint64_t> totals( nFields );
        std::vector<std::string> bytes( nFields );
        std::vector<std::vector<uint64_t> > offsets( nFields );
        std::string text;
        for ( uint64_t first = 0; rc == MI355X_BZ2_OK; first += WINDOW ) {
            uint64_t n = 0;
            rc = o.hasFieldQuote ? mi355x_bz2_reader_field_columns_quoted( reader, '\n', o.fieldDelimiter, o.cutFields.data(), (uint32_t)nFields,
                                                                           first, WINDOW, 0, &n, totals.data(), o.fieldQuote )
                                 : mi355x_bz2_reader_field_columns( reader, '\n', o.fieldDelimiter, o.cutFields.data(), (uint32_t)nFields,
                                                                    first, WINDOW, 0, &n, totals.data() );
            if ( rc != MI355X_BZ2_OK || n == 0 ) break;
            uint64_t total = 0;
            for ( size_t f = 0; f < nFields && rc == MI355X_BZ2_OK; ++f ) {
                bytes[f].resize( totals[f] );
                offsets[f].resize( n + 1 );
                rc = mi355x_bz2_reader_take_field_column( reader, (uint32_t)f, bytes[f].data(), offsets[f].data(), nullptr, 0 );
                total += totals[f];
            }
            if ( rc != MI355X_BZ2_OK ) break;
            text.clear();
            text.reserve( total + n * nFields );
            for ( uint64_t i = 0; i < n; ++i ) {
                for ( size_t f = 0; f < nFields; ++f ) {
                    text.append( bytes[f], offsets[f][i], offsets[f][i + 1] - offsets[f][i] );
                    text.push_back( f + 1 < nFields ? (char)o.fieldDelimiter : '\n' );
                }
            }
            std::cout << text;
            if ( n < WINDOW ) break;
        }
        if ( rc != MI355X_BZ2_OK ) {
            const char* detail = mi355x_bz2_reader_last_error( reader );
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( rc );
            if ( detail != nullptr && detail[0] != '\0' ) std::cerr << " (" << detail << ")";
            std::cerr << "\n";
            mi355x_bz2_reader_close( reader );
            return 1;
        }
        mi355x_bz2_reader_close( reader );
        return 0;
    }

    /* likewise an action of its own: the distinct values of one field with their counts, from the reader's field_groups;
     * the values of the groups come by read_ranges, in windows of groups */
    if ( o.countByField ) {
        Input in;
        if ( !in.open( o.input ) ) {
            std::cerr << "Could not open '" << o.input << "'\n";
            return 1;
        }
        if ( mi355x_bz2_read_stream_header( in.data, in.size, 0 ) == 0 ) {
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( MI355X_BZ2_ERR_STREAM_HEADER ) << "\n";
            return 1;
        }
        mi355x_bz2_reader* reader = nullptr;
        int rc = mi355x_bz2_reader_open_memory( in.data, in.size, o.decoderParallelism, o.device, &reader );
        if ( rc != MI355X_BZ2_OK ) {
            std::cerr << "Could not open the bzip2 stream: " << mi355x_bz2_status_string( rc ) << "\n";
            return 1;
        }
        uint64_t n = 0, missing = 0;
        rc = mi355x_bz2_reader_field_groups( reader, '\n', o.fieldDelimiter, o.field, o.seed, 0, ~uint64_t( 0 ), &n, &missing );
        std::vector<uint64_t> counts( n ), starts( n );
        std::vector<int64_t> sizes( n );
        if ( rc == MI355X_BZ2_OK ) rc = mi355x_bz2_reader_take_field_groups( reader, nullptr, counts.data(), starts.data(), sizes.data(), n );
        /* the groups ascend by first line: a stable sort by descending count keeps that order among equal counts */
        std::vector<uint64_t> order( n );
        for ( uint64_t i = 0; i < n; ++i ) order[i] = i;
        std::stable_sort( order.begin(), order.end(), [&counts] ( uint64_t a, uint64_t b ) { return counts[a] > counts[b]; } );
        constexpr uint64_t WINDOW = uint64_t( 1 ) << 20;
        std::vector<uint64_t> offsets, lengths, got;
        std::string bytes, text;
        for ( uint64_t first = 0; rc == MI355X_BZ2_OK && first < n; first += WINDOW ) {
            const uint64_t m = std::min( WINDOW, n - first );
            offsets.resize( m );
            lengths.resize( m );
            got.resize( m );
            uint64_t total = 0;
            for ( uint64_t i = 0; i < m; ++i ) {
                offsets[i] = starts[order[first + i]];
                total += lengths[i] = (uint64_t)sizes[order[first + i]];
            }
            bytes.resize( total );
            rc = mi355x_bz2_reader_read_ranges( reader, offsets.data(), lengths.data(), (uint32_t)m, bytes.data(), 0, got.data() );
            if ( rc != MI355X_BZ2_OK ) break;
            text.clear();
            uint64_t at = 0;
            for ( uint64_t i = 0; i < m; ++i ) {
                text += std::to_string( counts[order[first + i]] );
                text.push_back( '\t' );
                text.append( bytes, at, lengths[i] );
                text.push_back( '\n' );
                at += lengths[i];
            }
            std::cout << text;
        }
        if ( rc != MI355X_BZ2_OK ) {
            const char* detail = mi355x_bz2_reader_last_error( reader );
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( rc );
            if ( detail != nullptr && detail[0] != '\0' ) std::cerr << " (" << detail << ")";
            std::cerr << "\n";
            mi355x_bz2_reader_close( reader );
            return 1;
        }
        mi355x_bz2_reader_close( reader );
        return 0;
    }

    /* likewise an action of its own: the lines that a predicate on one field selects, from the reader's select_lines, printed
     * as --grep prints its lines */
    if ( o.whereField ) {
        std::string values = o.equals;
        std::vector<uint32_t> valueSizes;
        if ( o.whereEquals ) {
            if ( values.size() > 256 ) {
                std::cerr << "Bad value for --equals: more than 256 bytes\n";
                return 1;
            }
            valueSizes.push_back( (uint32_t)values.size() );
        } else if ( o.whereInFile ) {
            values.clear();
            if ( !readPatternFile( o.valueFile, values, valueSizes ) ) return 1;
            if ( valueSizes.empty() ) {
                std::cerr << "The value file '" << o.valueFile << "' holds no value\n";
                return 1;
            }
        }
        mi355x_bz2_regex* regex = nullptr;
        if ( o.whereMatches ) {
            /* before anything is opened, as --grep-regex has it */
            char why[512];
            if ( mi355x_bz2_regex_compile( reinterpret_cast<const uint8_t*>( o.matches.data() ), o.matches.size(), searchFlags, &regex,
                                           why, sizeof( why ) ) != MI355X_BZ2_OK ) {
                std::cerr << "Invalid regular expression: " << why << "\n";
                return 1;
            }
        }
        const std::unique_ptr<mi355x_bz2_regex, void ( * )( mi355x_bz2_regex* )> regexOwner( regex, mi355x_bz2_regex_free );
        Input in;
        if ( !in.open( o.input ) ) {
            std::cerr << "Could not open '" << o.input << "'\n";
            return 1;
        }
        if ( mi355x_bz2_read_stream_header( in.data, in.size, 0 ) == 0 ) {
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( MI355X_BZ2_ERR_STREAM_HEADER ) << "\n";
            return 1;
        }
        mi355x_bz2_reader* reader = nullptr;
        int rc = mi355x_bz2_reader_open_memory( in.data, in.size, o.decoderParallelism, o.device, &reader );
        if ( rc != MI355X_BZ2_OK ) {
            std::cerr << "Could not open the bzip2 stream: " << mi355x_bz2_status_string( rc ) << "\n";
            return 1;
        }
        uint64_t nLines = 0, total = 0;
        rc = o.whereMatches
             ? mi355x_bz2_reader_select_lines_regex( reader, '\n', o.fieldDelimiter, o.field, regex, o.invertMatch ? 1 : 0, 0, ~uint64_t( 0 ),
                                                     ~uint64_t( 0 ), 0, &nLines, &total )
             : mi355x_bz2_reader_select_lines( reader, '\n', o.fieldDelimiter, o.field, reinterpret_cast<const uint8_t*>( values.data() ),
                                               valueSizes.data(), (uint32_t)std::min<size_t>( valueSizes.size(), 0xFFFFFFFFu ), o.seed,
                                               o.hasLow ? 1 : 0, o.low, o.hasHigh ? 1 : 0, o.high, o.invertMatch ? 1 : 0, 0, ~uint64_t( 0 ),
                                               ~uint64_t( 0 ), 0, &nLines, &total );
        std::vector<uint64_t> numbers( nLines ), sizes( nLines );
        std::vector<char> bytes( total );
        if ( rc == MI355X_BZ2_OK ) rc = mi355x_bz2_reader_take_grep( reader, numbers.data(), sizes.data(), nLines );
        if ( rc == MI355X_BZ2_OK ) rc = mi355x_bz2_reader_take_line_ranges( reader, bytes.data(), 0 );
        if ( rc != MI355X_BZ2_OK ) {
            const char* detail = mi355x_bz2_reader_last_error( reader );
            std::cerr << "Selecting failed: " << mi355x_bz2_status_string( rc );
            if ( detail != nullptr && detail[0] != '\0' ) std::cerr << " (" << detail << ")";
            std::cerr << "\n";
            mi355x_bz2_reader_close( reader );
            return 1;
        }
        mi355x_bz2_reader_close( reader );
        if ( !o.lineNumber ) {
            std::cout.write( bytes.data(), (std::streamsize)bytes.size() );
        } else {
            uint64_t at = 0;
            for ( uint64_t i = 0; i < nLines; at += sizes[i], ++i ) {
                std::cout << numbers[i] + 1 << ':';
                std::cout.write( bytes.data() + at, (std::streamsize)sizes[i] );
            }
        }
        std::cout.flush();
        return std::cout.good() ? 0 : 1;
    }

    /* likewise an action of its own: the sum of one field per distinct value of another, from the reader's field_sums; the
     * keys of the groups come by read_ranges, in windows of groups */
    if ( o.sumByField ) {
        Input in;
        if ( !in.open( o.input ) ) {
            std::cerr << "Could not open '" << o.input << "'\n";
            return 1;
        }
        if ( mi355x_bz2_read_stream_header( in.data, in.size, 0 ) == 0 ) {
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( MI355X_BZ2_ERR_STREAM_HEADER ) << "\n";
            return 1;
        }
        mi355x_bz2_reader* reader = nullptr;
        int rc = mi355x_bz2_reader_open_memory( in.data, in.size, o.decoderParallelism, o.device, &reader );
        if ( rc != MI355X_BZ2_OK ) {
            std::cerr << "Could not open the bzip2 stream: " << mi355x_bz2_status_string( rc ) << "\n";
            return 1;
        }
        uint64_t n = 0, missing = 0;
        rc = mi355x_bz2_reader_field_sums( reader, '\n', o.fieldDelimiter, o.field, o.valueField, o.seed, 0, ~uint64_t( 0 ), &n, &missing );
        std::vector<uint64_t> starts( n ), numbers( n ), low( n );
        std::vector<int64_t> sizes( n ), high( n );
        if ( rc == MI355X_BZ2_OK ) {
            rc = mi355x_bz2_reader_take_field_sums( reader, nullptr, nullptr, starts.data(), sizes.data(), numbers.data(), low.data(),
                                                    high.data(), nullptr, nullptr, n );
        }
        /* hi * 2^64 + lo in decimal */
        const auto decimal = [] ( int64_t hi, uint64_t lo ) {
            const __int128 value = (__int128)( ( (unsigned __int128)(uint64_t)hi << 64 ) | lo );
            unsigned __int128 magnitude = value < 0 ? -(unsigned __int128)value : (unsigned __int128)value;
            std::string digits;
            do {
                digits.push_back( (char)( '0' + (int)( magnitude % 10 ) ) );
                magnitude /= 10;
            } while ( magnitude != 0 );
            if ( value < 0 ) digits.push_back( '-' );
            return std::string( digits.rbegin(), digits.rend() );
        };
        constexpr uint64_t WINDOW = uint64_t( 1 ) << 20;
        std::vector<uint64_t> lengths, got;
        std::string bytes, text;
        for ( uint64_t first = 0; rc == MI355X_BZ2_OK && first < n; first += WINDOW ) {
            const uint64_t m = std::min( WINDOW, n - first );
            lengths.resize( m );
            got.resize( m );
            uint64_t total = 0;
            for ( uint64_t i = 0; i < m; ++i ) total += lengths[i] = (uint64_t)sizes[first + i];
            bytes.resize( total );
            rc = mi355x_bz2_reader_read_ranges( reader, starts.data() + first, lengths.data(), (uint32_t)m, bytes.data(), 0, got.data() );
            if ( rc != MI355X_BZ2_OK ) break;
            text.clear();
            uint64_t at = 0;
            for ( uint64_t i = 0; i < m; ++i ) {
                text += decimal( high[first + i], low[first + i] );
                text.push_back( '\t' );
                text += std::to_string( numbers[first + i] );
                text.push_back( '\t' );
                text.append( bytes, at, lengths[i] );
                text.push_back( '\n' );
                at += lengths[i];
            }
            std::cout << text;
        }
        if ( rc != MI355X_BZ2_OK ) {
            const char* detail = mi355x_bz2_reader_last_error( reader );
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( rc );
            if ( detail != nullptr && detail[0] != '\0' ) std::cerr << " (" << detail << ")";
            std::cerr << "\n";
            mi355x_bz2_reader_close( reader );
            return 1;
        }
        mi355x_bz2_reader_close( reader );
        return 0;
    }

    /* likewise an action of its own: the number of matches of a string in the decoded data, from the reader's search */
    if ( o.countMatches ) {
        Input in;
        if ( !in.open( o.input ) ) {
            std::cerr << "Could not open '" << o.input << "'\n";
            return 1;
        }
        if ( mi355x_bz2_read_stream_header( in.data, in.size, 0 ) == 0 ) {
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( MI355X_BZ2_ERR_STREAM_HEADER ) << "\n";
            return 1;
        }
        mi355x_bz2_reader* reader = nullptr;
        int rc = mi355x_bz2_reader_open_memory( in.data, in.size, o.decoderParallelism, o.device, &reader );
        if ( rc != MI355X_BZ2_OK ) {
            std::cerr << "Could not open the bzip2 stream: " << mi355x_bz2_status_string( rc ) << "\n";
            return 1;
        }
        uint64_t count = 0;
        rc = mi355x_bz2_reader_search_ex( reader, reinterpret_cast<const uint8_t*>( o.pattern.data() ), (uint32_t)o.pattern.size(),
                                          searchFlags, 0, ~uint64_t( 0 ), 0, &count );
        if ( rc != MI355X_BZ2_OK ) {
            const char* detail = mi355x_bz2_reader_last_error( reader );
            std::cerr << "Search failed: " << mi355x_bz2_status_string( rc );
            if ( detail != nullptr && detail[0] != '\0' ) std::cerr << " (" << detail << ")";
            std::cerr << "\n";
            mi355x_bz2_reader_close( reader );
            return 1;
        }
        mi355x_bz2_reader_close( reader );
        std::cout << count << "\n";
        return 0;
    }

    /* likewise: the lines that hold a match (bzgrep -F), from the reader's grep, or that match a regular expression
     * (bzgrep), from its grep_regex; 0 also when no line matched */
    if ( o.grep || o.grepRegex ) {
        mi355x_bz2_regex* regex = nullptr;
        if ( o.grepRegex ) {
            /* before anything is opened: a pattern outside the syntax is the user's to fix */
            char why[512];
            if ( mi355x_bz2_regex_compile( reinterpret_cast<const uint8_t*>( o.regex.data() ), o.regex.size(), searchFlags, &regex,
                                           why, sizeof( why ) ) != MI355X_BZ2_OK ) {
                std::cerr << "Invalid regular expression: " << why << "\n";
                return 1;
            }
        }
        const std::unique_ptr<mi355x_bz2_regex, void ( * )( mi355x_bz2_regex* )> regexOwner( regex, mi355x_bz2_regex_free );
        Input in;
        if ( !in.open( o.input ) ) {
            std::cerr << "Could not open '" << o.input << "'\n";
            return 1;
        }
        if ( mi355x_bz2_read_stream_header( in.data, in.size, 0 ) == 0 ) {
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( MI355X_BZ2_ERR_STREAM_HEADER ) << "\n";
            return 1;
        }
        mi355x_bz2_reader* reader = nullptr;
        int rc = mi355x_bz2_reader_open_memory( in.data, in.size, o.decoderParallelism, o.device, &reader );
        if ( rc != MI355X_BZ2_OK ) {
            std::cerr << "Could not open the bzip2 stream: " << mi355x_bz2_status_string( rc ) << "\n";
            return 1;
        }
        uint64_t nLines = 0, total = 0;
        rc = o.grepRegex
             ? mi355x_bz2_reader_grep_regex( reader, regex, '\n', ~uint64_t( 0 ), 0, &nLines, &total )
             : mi355x_bz2_reader_grep_ex( reader, reinterpret_cast<const uint8_t*>( o.pattern.data() ), (uint32_t)o.pattern.size(),
                                          searchFlags, '\n', 0, ~uint64_t( 0 ), ~uint64_t( 0 ), 0, &nLines, &total );
        std::vector<uint64_t> numbers( nLines ), sizes( nLines );
        std::vector<char> bytes( total );
        if ( rc == MI355X_BZ2_OK ) rc = mi355x_bz2_reader_take_grep( reader, numbers.data(), sizes.data(), nLines );
        if ( rc == MI355X_BZ2_OK ) rc = mi355x_bz2_reader_take_line_ranges( reader, bytes.data(), 0 );
        if ( rc != MI355X_BZ2_OK ) {
            const char* detail = mi355x_bz2_reader_last_error( reader );
            std::cerr << "Search failed: " << mi355x_bz2_status_string( rc );
            if ( detail != nullptr && detail[0] != '\0' ) std::cerr << " (" << detail << ")";
            std::cerr << "\n";
            mi355x_bz2_reader_close( reader );
            return 1;
        }
        mi355x_bz2_reader_close( reader );
        if ( !o.lineNumber ) {
            std::cout.write( bytes.data(), (std::streamsize)bytes.size() );
        } else {
            uint64_t at = 0;
            for ( uint64_t i = 0; i < nLines; at += sizes[i], ++i ) {
                std::cout << numbers[i] + 1 << ':';
                std::cout.write( bytes.data() + at, (std::streamsize)sizes[i] );
            }
        }
        std::cout.flush();
        return std::cout.good() ? 0 : 1;
    }

    /* the same two actions for a set of strings, from the reader's search_set and grep_set */
    if ( o.grepFile || o.countMatchesFile ) {
        std::string patterns;
        std::vector<uint32_t> patternSizes;
        if ( !readPatternFile( o.patternFile, patterns, patternSizes ) ) return 1;
        Input in;
        if ( !in.open( o.input ) ) {
            std::cerr << "Could not open '" << o.input << "'\n";
            return 1;
        }
        if ( mi355x_bz2_read_stream_header( in.data, in.size, 0 ) == 0 ) {
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( MI355X_BZ2_ERR_STREAM_HEADER ) << "\n";
            return 1;
        }
        mi355x_bz2_reader* reader = nullptr;
        int rc = mi355x_bz2_reader_open_memory( in.data, in.size, o.decoderParallelism, o.device, &reader );
        if ( rc != MI355X_BZ2_OK ) {
            std::cerr << "Could not open the bzip2 stream: " << mi355x_bz2_status_string( rc ) << "\n";
            return 1;
        }
        const auto* const set = reinterpret_cast<const uint8_t*>( patterns.data() );
        const auto nPatterns = (uint32_t)std::min<size_t>( patternSizes.size(), 0xFFFFFFFFu );
        uint64_t nLines = 0, total = 0, nMatches = 0;
        std::vector<uint64_t> numbers, sizes, each( patternSizes.size() );
        std::vector<char> bytes;
        if ( o.countMatchesFile ) {
            rc = mi355x_bz2_reader_search_set_ex( reader, set, patternSizes.data(), nPatterns, searchFlags, 0, ~uint64_t( 0 ), 0,
                                                  &nMatches, each.data() );
        } else {
            rc = mi355x_bz2_reader_grep_set_ex( reader, set, patternSizes.data(), nPatterns, searchFlags, '\n', 0, ~uint64_t( 0 ),
                                                ~uint64_t( 0 ), 0, &nLines, &total );
            numbers.resize( nLines );
            sizes.resize( nLines );
            bytes.resize( total );
            if ( rc == MI355X_BZ2_OK ) rc = mi355x_bz2_reader_take_grep( reader, numbers.data(), sizes.data(), nLines );
            if ( rc == MI355X_BZ2_OK ) rc = mi355x_bz2_reader_take_line_ranges( reader, bytes.data(), 0 );
        }
        if ( rc != MI355X_BZ2_OK ) {
            const char* detail = mi355x_bz2_reader_last_error( reader );
            std::cerr << "Search failed: " << mi355x_bz2_status_string( rc );
            if ( detail != nullptr && detail[0] != '\0' ) std::cerr << " (" << detail << ")";
            std::cerr << "\n";
            mi355x_bz2_reader_close( reader );
            return 1;
        }
        mi355x_bz2_reader_close( reader );
        if ( o.countMatchesFile ) {
            for ( const auto count : each ) std::cout << count << "\n";
        } else if ( !o.lineNumber ) {
            std::cout.write( bytes.data(), (std::streamsize)bytes.size() );
        } else {
            uint64_t at = 0;
            for ( uint64_t i = 0; i < nLines; at += sizes[i], ++i ) {
                std::cout << numbers[i] + 1 << ':';
                std::cout.write( bytes.data() + at, (std::streamsize)sizes[i] );
            }
        }
        std::cout.flush();
        return std::cout.good() ? 0 : 1;
    }

    /* output file name rules, ibzip2.cpp:316-331 */
    std::string outputPath = o.output;
    if ( !o.toStdout && outputPath.empty() && !o.input.empty() ) {
        if ( endsWithNoCase( o.input, ".bz2" ) ) {
            outputPath = o.input.substr( 0, o.input.size() - 4 );
        } else {
            outputPath = o.input + ".out";
            if ( !o.quiet ) std::cerr << "Could not deduce output file name. Will write to '" << outputPath << "'\n";
        }
    }
    if ( o.verbose > 0 ) {
        const auto show = [] ( const std::string& v, bool given ) { return v.empty() ? ( given ? "<stdout>" : "<none>" ) : v.c_str(); };
        std::cerr << "file path for input: " << show( o.input, false ) << "\n"
                  << "file path for output: " << show( o.output, o.hasOutput ) << "\n"
                  << "file path for list-compressed-offsets: " << show( o.listCompressedPath, o.listCompressed ) << "\n"
                  << "file path for list-offsets: " << show( o.listOffsetsPath, o.listOffsets ) << "\n";
    }
    if ( o.decompress && outputPath != "/dev/null" && !outputPath.empty() && fileExists( outputPath ) && !o.force ) {
        std::cerr << "Output file '" << outputPath << "' already exists! Use --force to overwrite.\n";
        return 1;
    }
    if ( !o.listOffsetsPath.empty() && fileExists( o.listOffsetsPath ) && !o.force ) {
        std::cerr << "Output file for offsets'" << o.listOffsetsPath << "' for offsets already exists! Use --force to overwrite.\n";
        return 1;
    }
    if ( !o.listCompressedPath.empty() && fileExists( o.listCompressedPath ) && !o.force ) {
        std::cerr << "Output file compressed offsets '" << o.listCompressedPath
                  << "' for offsets already exists! Use --force to overwrite.\n";
        return 1;
    }

    if ( o.decompress || o.listOffsets ) {
        if ( o.verbose > 0 ) {
            std::cerr << "Decompress " << o.input << " -> " << outputPath << " with " << o.decoderParallelism
                      << " blocks per GPU batch\n";
        }
        Input in;
        if ( !in.open( o.input ) ) {
            std::cerr << "Could not open '" << o.input << "'\n";
            return 1;
        }
        /* the reference's default (serial) reader starts with readBzip2Header (bzip2.hpp:114-142) and throws on
         * anything else; its parallel reader would silently produce nothing for an input without a block magic */
        if ( mi355x_bz2_read_stream_header( in.data, in.size, 0 ) == 0 ) {
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( MI355X_BZ2_ERR_STREAM_HEADER ) << "\n";
            return 1;
        }
        int outFd = -1;
        bool writingToStdout = false;
        if ( o.decompress ) {
            if ( outputPath.empty() ) {
                outFd = STDOUT_FILENO;
                writingToStdout = true;
            } else {
                outFd = ::open( outputPath.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644 );
                if ( outFd < 0 ) {
                    std::cerr << "Could not open output file '" << outputPath << "' for writing!\n";
                    return 1;
                }
            }
        }

        const auto tOpen = std::chrono::steady_clock::now();
        mi355x_bz2_reader* reader = nullptr;
        int rc = mi355x_bz2_reader_open_memory( in.data, in.size, o.decoderParallelism, o.device, &reader );
        if ( rc != MI355X_BZ2_OK ) {
            std::cerr << "Could not open the bzip2 stream: " << mi355x_bz2_status_string( rc ) << "\n";
            if ( outFd >= 0 && !writingToStdout ) ::close( outFd );
            return 1;
        }
        if ( o.test ) (void)mi355x_bz2_reader_set_verify_stream_crc( reader, 1 );
        const auto fail = [&] ( int status ) {
            const char* detail = mi355x_bz2_reader_last_error( reader );
            std::cerr << "Decoding failed: " << mi355x_bz2_status_string( status );
            if ( detail != nullptr && detail[0] != '\0' ) std::cerr << " (" << detail << ")";
            std::cerr << "\n";
            mi355x_bz2_reader_close( reader );
            if ( outFd >= 0 && !writingToStdout ) ::close( outFd );
            return 1;
        };

        const auto tRead = std::chrono::steady_clock::now();
        uint64_t written = 0;
        if ( o.bufferSize > 0 ) {
            std::vector<char> buffer( o.bufferSize );
            do {
                uint64_t got = 0;
                rc = mi355x_bz2_reader_read( reader, -1, buffer.data(), buffer.size(), &got );
                if ( rc != MI355X_BZ2_OK ) return fail( rc );
                if ( outFd >= 0 ) {
                    uint64_t done = 0;
                    while ( done < got ) {
                        const ssize_t n = ::write( outFd, buffer.data() + done, got - done );
                        if ( n < 0 && errno == EINTR ) continue;
                        if ( n <= 0 ) {
                            std::cerr << "Could not write all the decoded data to the specified output!\n";
                            break;
                        }
                        done += (uint64_t)n;
                    }
                }
                written += got;
            } while ( !mi355x_bz2_reader_eof( reader ) );
        } else {
            rc = mi355x_bz2_reader_read( reader, outFd, nullptr, UINT64_MAX, &written );
            if ( rc != MI355X_BZ2_OK ) return fail( rc );
        }
        if ( outFd >= 0 && !writingToStdout ) ::close( outFd );
        const auto tDone = std::chrono::steady_clock::now();

        std::ostream& out = writingToStdout ? std::cerr : std::cout;

        uint64_t count = 0;
        rc = mi355x_bz2_reader_block_offsets( reader, nullptr, nullptr, 0, &count );
        if ( rc != MI355X_BZ2_OK ) return fail( rc );
        std::vector<uint64_t> bits( count ), bytes( count );
        rc = mi355x_bz2_reader_block_offsets( reader, bits.data(), bytes.data(), count, &count );
        if ( rc != MI355X_BZ2_OK ) return fail( rc );
        if ( o.verbose > 0 ) out << "Found " << count << " blocks\n";

        if ( o.test ) {
            /* the final entry of the map is the end-of-file sentinel, not a magic (BlockMap.hpp:207-230) */
            std::vector<uint64_t> magics( bits.begin(), bits.end() - ( bits.empty() ? 0 : 1 ) );
            if ( !checkOffsets( in, magics ) ) { mi355x_bz2_reader_close( reader ); return 1; }
            uint64_t size = 0;
            if ( !mi355x_bz2_reader_size( reader, &size ) ) {
                std::cerr << "Bzip2 reader size should be available at this point!\n";
                mi355x_bz2_reader_close( reader );
                return 1;
            }
            if ( written != size ) {
                std::cerr << "Wrote less bytes (" << written << " B) than decoded stream is large(" << size << " B)!\n";
                mi355x_bz2_reader_close( reader );
                return 1;
            }
        }
        if ( o.verbose > 1 ) {
            mi355x_bz2_reader_stats st{};
            if ( mi355x_bz2_reader_statistics( reader, &st ) == MI355X_BZ2_OK ) {
                std::cerr << "[statistics] gets " << st.gets << ", cache hits " << st.cache_hits << ", prefetch hits "
                          << st.prefetch_hits << ", on-demand " << st.on_demand_fetches << ", GPU batches " << st.batches
                          << ", blocks decoded " << st.blocks_decoded << ", decode " << st.decode_seconds << " s, wait "
                          << st.wait_seconds << " s\n";
            }
        }
        mi355x_bz2_reader_close( reader );
        if ( o.verbose > 1 ) {
            const auto seconds = [] ( auto a, auto b ) { return std::chrono::duration<double>( b - a ).count(); };
            std::cerr << "[timing] open " << seconds( tOpen, tRead ) << " s, decode " << seconds( tRead, tDone )
                      << " s, close " << seconds( tDone, std::chrono::steady_clock::now() ) << " s\n";
        }

        if ( o.listOffsets ) {
            if ( !o.listOffsetsPath.empty() ) {
                std::ofstream file( o.listOffsetsPath );
                dumpOffsets( file, bits, bytes );
            } else if ( outputPath.empty() ) {
                dumpOffsets( std::cerr, bits, bytes );
            } else {
                dumpOffsets( std::cout, bits, bytes );
            }
        }
        if ( o.listCompressed ) {
            if ( !o.listCompressedPath.empty() ) {
                std::ofstream file( o.listCompressedPath );
                dumpOffsets( file, bits );
            } else if ( outputPath.empty() ) {
                dumpOffsets( std::cerr, bits );
            } else {
                dumpOffsets( std::cout, bits );
            }
        }
        return 0;
    }

    if ( o.listCompressed ) {
        if ( o.verbose > 0 ) std::cerr << "Find block offsets\n";
        return findCompressedBlocks( o );
    }

    std::cerr << "No suitable arguments were given. Please refer to the help!\n\n";
    printHelp();
    return 1;
}
