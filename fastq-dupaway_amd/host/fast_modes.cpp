// fast_modes.cpp — the FQD_FAST_* switches: the one place each is read, what they refuse, and how the messages name them.
#include "fast_modes.hpp"
#include <cstdlib>
#include <cstring>
#include <utility>
#include "fqdupaway.h"

namespace fqdhost {
namespace detail {

namespace {

// NAME=1 (any integer but 0) turns a switch on.
bool is_on(const char* name) { const char* v = std::getenv(name); return v && std::atoi(v) != 0; }

// The place of the variable's value among `spellings` (unset: 0, the default's); `must_be` words the error.
template <size_t N>
int choice(const char* name, const char* const (&spellings)[N], const char* must_be)
{
    const char* v = std::getenv(name);
    if (!v) return 0;
    for (size_t k = 0; k < N; ++k) if (std::strcmp(v, spellings[k]) == 0) return int(k);
    throw std::runtime_error(std::string(name) + " must be " + must_be + ", not '" + v + "'");
}

uint32_t size_bound(const char* name, uint32_t unset)
{
    const char* v = std::getenv(name);
    if (!v) return unset;
    uint64_t x = 0;
    size_t digits = 0;
    for (const char* p = v; *p; ++p, ++digits) {
        if (*p < '0' || *p > '9' || digits >= 10) { digits = 0; break; }
        x = x * 10 + uint64_t(*p - '0');
    }
    if (!digits || x < 1 || x > 0x7FFFFFFFull)
        throw std::runtime_error(std::string(name) + " must be a decimal integer in 1 .. 2147483647, not '" + v + "'");
    return uint32_t(x);
}

// FQD_FAST_OPTICAL: size_bound's values, and 0 (like unset) for off.
uint32_t pixel_distance(const char* name)
{
    const char* v = std::getenv(name);
    if (!v) return 0;
    bool zero = *v != 0;
    for (const char* p = v; *p && zero; ++p) zero = *p == '0' && p - v < 10;
    return zero ? 0 : size_bound(name, 0);
}

// FQD_FAST_PREFIX: a decimal integer in 1 .. 65535, and 0 (like unset) for off.
uint32_t min_overlap(const char* name)
{
    const char* v = std::getenv(name);
    if (!v) return 0;
    uint32_t x = 0;
    size_t digits = 0;
    for (const char* p = v; *p; ++p, ++digits) {
        if (*p < '0' || *p > '9' || digits >= 5) { digits = 0; break; }
        x = x * 10 + uint32_t(*p - '0');
    }
    if (!digits || x > 65535 || (digits > 1 && v[0] == '0'))
        throw std::runtime_error(std::string(name) + " must be a decimal integer in 1 .. 65535 (or 0 for off), not '" + v + "'");
    return x;
}

} // namespace

FastModes FastModes::from_env()
{
    FastModes m;
    m.keep_best = choice("FQD_FAST_KEEP", {"first", "best"}, "'first' or 'best'") == 1;
    m.sort_by_size = choice("FQD_FAST_SORT", {"input", "size"}, "'input' or 'size'") == 1;
    m.min_size = size_bound("FQD_FAST_MINSIZE", 1);
    m.max_size = size_bound("FQD_FAST_MAXSIZE", 0);
    if (m.max_size && m.max_size < m.min_size)
        throw FastModeRefusal("FQD_FAST_MAXSIZE=" + std::to_string(m.max_size) + " is below FQD_FAST_MINSIZE=" + std::to_string(m.min_size) + ": no cluster could be written");
    m.clusters = is_on("FQD_FAST_CLUSTERS");
    m.both_strands = choice("FQD_FAST_STRAND", {"given", "both"}, "'given' or 'both'") == 1;
    const int separator[3] = {0, ':', '_'};
    m.umi = separator[choice("FQD_FAST_UMI", {"off", "colon", "underscore"}, "'off', 'colon' or 'underscore'")];
    m.umi_mismatch = choice("FQD_FAST_UMI_MISMATCH", {"0", "1", "2"}, "0, 1 or 2");
    m.size_out = is_on("FQD_FAST_SIZEOUT");
    m.levels = is_on("FQD_FAST_LEVELS");
    m.size_in = is_on("FQD_FAST_SIZEIN");
    m.optical = pixel_distance("FQD_FAST_OPTICAL");
    m.hamming = uint32_t(choice("FQD_FAST_HAMMING", {"0", "1", "2", "3"}, "0, 1, 2 or 3"));
    m.umi_hamming = uint32_t(choice("FQD_FAST_UMI_HAMMING", {"0", "1", "2", "3"}, "0, 1, 2 or 3"));
    const char* centroid = std::getenv("FQD_FAST_CENTROID");
    m.longest = centroid && std::strcmp(centroid, "longest") == 0;
    if (!m.longest) m.centroid = choice("FQD_FAST_CENTROID", {"first", "abundant"}, "'first' or 'abundant'") == 1;
    m.consensus = is_on("FQD_FAST_CONSENSUS");
    m.prefix = min_overlap("FQD_FAST_PREFIX");
    return m;
}

std::string FastModes::names() const
{
    // (min_size 1 and max_size 0 are the two bounds that take nothing out: not named)
    const std::pair<bool, std::string> all[] = {
        {keep_best, "FQD_FAST_KEEP=best"}, {clusters, "FQD_FAST_CLUSTERS=1"}, {both_strands, "FQD_FAST_STRAND=both"}, {umi != 0, umi_name()}, {umi_mismatch != 0, mismatch_name()},
        {umi_hamming != 0, umi_hamming_name()},
        {hamming != 0, hamming_name()},
        {optical != 0, optical_name()},
        {consensus, "FQD_FAST_CONSENSUS=1"},
        {centroid, "FQD_FAST_CENTROID=abundant"}, {longest, "FQD_FAST_CENTROID=longest"},
        {size_out, "FQD_FAST_SIZEOUT=1"}, {levels, "FQD_FAST_LEVELS=1"}, {sort_by_size, "FQD_FAST_SORT=size"}, {size_in, "FQD_FAST_SIZEIN=1"},
        {min_size > 1, "FQD_FAST_MINSIZE=" + std::to_string(min_size)}, {max_size != 0, "FQD_FAST_MAXSIZE=" + std::to_string(max_size)},
        {prefix != 0, prefix_name()}};
    std::string s;
    for (const auto& one : all) if (one.first) s += (s.empty() ? "" : " and ") + one.second;
    return s;
}

void FastModes::check(bool unordered, size_t n_devices, Format format) const
{
    if (size_in && !sized())
        throw FastModeRefusal("FQD_FAST_SIZEIN=1 changes what a cluster's size is and nothing else: set one of FQD_FAST_SIZEOUT=1, FQD_FAST_LEVELS=1, FQD_FAST_SORT=size, "
                              "FQD_FAST_MINSIZE (above 1) or FQD_FAST_MAXSIZE as well, which read the sizes");
    if (!any()) return;
    if (umi_mismatch && !umi)
        throw FastModeRefusal(mismatch_name() + " merges the UMIs that FQD_FAST_UMI finds: set FQD_FAST_UMI=colon or FQD_FAST_UMI=underscore as well");
    if (hamming && both_strands)
        throw FastModeRefusal(hamming_name() + " with FQD_FAST_STRAND=both: a substituted base can change which orientation of a read is the canonical one, so copies with errors "
                              "may be keyed in opposite orientations and never be compared");
    if (hamming && umi)
        throw FastModeRefusal(hamming_name() + " with " + umi_name() + (umi_mismatch ? " and " + mismatch_name() : std::string()) +
                              ": which sequences under one UMI are copies of one molecule is a rule of its own, and this switch merges by sequence alone");
    if (umi_hamming && !umi)
        throw FastModeRefusal(umi_hamming_name() + " merges the sequences under one of the UMIs that FQD_FAST_UMI finds: set FQD_FAST_UMI=colon or FQD_FAST_UMI=underscore as well");
    if (umi_hamming && both_strands)
        throw FastModeRefusal(umi_hamming_name() + " with FQD_FAST_STRAND=both: a substituted base can change which orientation of a read is the canonical one, so copies with errors "
                              "may be keyed in opposite orientations and never be compared");
    if (consensus && both_strands)
        throw FastModeRefusal("FQD_FAST_CONSENSUS=1 with FQD_FAST_STRAND=both: the members of a cluster may be keyed in opposite orientations, and a column-wise vote "
                              "needs them in one; turning reads for the vote is not done");
    if (consensus && size_in)
        throw FastModeRefusal("FQD_FAST_CONSENSUS=1 with FQD_FAST_SIZEIN=1: a record that stands for several reads has lost the quality lines of the reads it stands "
                              "for, and the vote weighs every base by its quality");
    if (centroid && !merges())
        throw FastModeRefusal("FQD_FAST_CENTROID=abundant chooses among the different sequences of a merged cluster and nothing else: set one of FQD_FAST_UMI_MISMATCH, "
                              "FQD_FAST_HAMMING or FQD_FAST_UMI_HAMMING as well, which merge them (without one every cluster holds one sequence)");
    if (unordered)
        throw FastModeRefusal(names() + " with --unordered: these modes run on ordered inputs only");
    if (n_devices > 1)
        throw FastModeRefusal(names() + " runs on one GPU: FQD_DEVICES may name one device only");
    if (keep_best && format == Format::Fasta)
        throw FastModeRefusal("FQD_FAST_KEEP=best needs the quality lines of FASTQ records: --format fasta has none");
    if (consensus && format == Format::Fasta)
        throw FastModeRefusal("FQD_FAST_CONSENSUS=1 with --format fasta: the vote weighs every base by its quality, and FASTA records have no quality lines");
    if (prefix && hamming)
        throw FastModeRefusal(prefix_name() + " with " + hamming_name() + ": a truncated copy with substituted bases inside the overlap is a rule of its own, and each of the "
                              "two switches merges by its own rule alone");
    if (prefix && umi)
        throw FastModeRefusal(prefix_name() + " with " + umi_name() + (umi_mismatch ? " and " + mismatch_name() : std::string()) + (umi_hamming ? " and " + umi_hamming_name() : std::string()) +
                              ": which sequences under one UMI are copies of one molecule is a rule of its own, and this switch merges by sequence alone");
    if (prefix && both_strands)
        throw FastModeRefusal(prefix_name() + " with FQD_FAST_STRAND=both: a truncated read's reverse complement is a suffix of its untrimmed copy's, not a prefix, so the two "
                              "would be keyed in orientations that are never compared");
    if (prefix && consensus)
        throw FastModeRefusal(prefix_name() + " with FQD_FAST_CONSENSUS=1: the members of a merged cluster differ in length, and a column-wise vote needs members of one length");
    if (longest && !prefix)
        throw FastModeRefusal("FQD_FAST_CENTROID=longest chooses the sequence that all others of a merged cluster are prefixes of, and nothing else: set FQD_FAST_PREFIX as well, "
                              "which merges them (FQD_FAST_CENTROID=abundant goes with the other merging switches)");
}

std::string FastModes::out_of_memory_note() const
{
    // what every run holds, what the key rewrites add, and the links
    std::string s = "the text, the record arrays";
    if (umi) s += ", the keyed bytes of FQD_FAST_UMI (mate 1's sequence bytes once more and the UMI bases of every record, 16 bytes a record)";
    if (both_strands) s += ", the canonical reads (the sequence bytes once more, 12 bytes a record and mate, 1 byte a record)";
    s += umi || both_strands ? " and, with FQD_FAST_KEEP / FQD_FAST_CLUSTERS," : " and";
    s += " up to 37 bytes a record for the links, the owners and their grouping do not fit in GPU memory";
    // what the size switches, the order and the mismatch switch add, named only when one of them is set
    if (sized()) {
        s += std::string("; the cluster sizes of ") + (size_out ? "FQD_FAST_SIZEOUT" : levels ? "FQD_FAST_LEVELS" : sort_by_size ? "FQD_FAST_SORT" : "FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE") +
             " take 4 bytes a record more";
        if (size_out) s += " and the labels' places and grown sizes 8 bytes a record and file";
        if (size_in) s += "; FQD_FAST_SIZEIN takes 4 bytes a record for the weights while the sizes are made";
        if (size_in && size_out) s += " and 4 bytes a record and file for the annotations' lengths in the writer";
    }
    if (sort_by_size) {
        s += "; FQD_FAST_SORT=size takes 4 bytes a cluster for the written order, 1 byte a cluster for its flags and, while it sorts, "
             "24 bytes a cluster of scratch (the scratch of the grouping serves where it is as large)";
        if (size_out) s += ", and the labels' places and the sizes in written order 4 bytes a cluster and file and 4 bytes a cluster";
    }
    if (umi_mismatch)
        s += "; FQD_FAST_UMI_MISMATCH takes 12 bytes a record more (the owners by sequence, the exact counts, the merged owners) "
             "and, while it merges, 4 bytes a record and up to 66 bytes an exact cluster";
    if (hamming)
        s += "; FQD_FAST_HAMMING takes 4 bytes a record for the merged owners and, while it merges, " + std::to_string(24 * (hamming + 1)) +
             " bytes an exact cluster for the seeds and their sort (12 bytes a seed, " + std::to_string(hamming + 1) +
             " seeds a cluster, twice over), 4 bytes a record for the labels and 8 bytes for every pair of clusters found near, with room for " +
             std::to_string(hamming + 1) + " such pairs a cluster from the start";
    if (umi_hamming)
        s += "; FQD_FAST_UMI_HAMMING takes 4 bytes a record for the molecules' owners" + std::string(umi_mismatch ? ", 4 bytes a record more for the exact owners kept beside the merged ones" : "") +
             " and, while it merges, " + std::to_string(24 * (umi_hamming + 1)) + " bytes an exact cluster for the seeds and their sort, 4 bytes a record for the labels and 8 bytes for every "
             "pair of clusters found near" + (umi_mismatch ? " and every link" : "") + ", with room for " + std::to_string(umi_hamming + 1) + " of them a cluster from the start";
    if (optical)
        s += "; FQD_FAST_OPTICAL takes 16 bytes a record for the places (tile, x, y, surface) and 4 for the split owners and, while it splits, "
             "up to 17 bytes a record of scratch (the scratch of the grouping serves where it is as large)";
    if (consensus)
        s += "; FQD_FAST_CONSENSUS takes, for paired files, 1 byte a record for the pairs it changed and, while it votes, 4 bytes a cluster and up to 5 bytes a "
             "record of scratch (the scratch of the grouping serves where it is as large)";
    if (centroid)
        s += "; FQD_FAST_CENTROID takes 4 bytes a record for the exact owners kept beside the merged ones and, while it chooses, 4 bytes a record for the "
             "abundances, about 5 bytes a record of scratch and 32 bytes for every member of a cluster above 2048";
    if (prefix)
        s += "; FQD_FAST_PREFIX takes 4 bytes a record for the merged owners and, while it merges, 24 bytes an exact cluster for the seeds and their sort (12 bytes a seed, "
             "one seed a cluster of at least " + std::to_string(prefix) + " bases a mate, twice over), 8 bytes a record for the parents and 4 bytes a record for the roots";
    if (longest)
        s += "; FQD_FAST_CENTROID=longest takes 4 bytes a record for the exact owners kept beside the merged ones and 4 bytes a record for the lengths, and, while it chooses, "
             "about 5 bytes a record of scratch";
    return s;
}

std::string umi_reason(uint32_t reason, int sep)
{
    const std::string c(1, char(sep));
    switch (reason) {
    case FQD_UMI_NO_SEPARATOR: return "the first word of its ID line holds no '" + c + "'";
    case FQD_UMI_EMPTY: return "its UMI is empty: the last '" + c + "' is the last byte of the ID line's first word";
    case FQD_UMI_TOO_LONG: return "its UMI is longer than 64 bytes";
    case FQD_UMI_BAD_BYTE: return "its UMI holds a byte outside ACGTN+-_";
    case FQD_UMI_NO_BASE: return "its UMI has no base";
    case FQD_UMI_SHAPE_DIFFERS: return "the shape of its UMI (its length and the places of '+', '-', '_') differs from record 0's: UMIs of varying length are not supported";
    }
    return "its UMI was refused";
}

std::string optical_reason(uint32_t reason)
{
    switch (reason) {
    case FQD_PLACE_FEW_FIELDS: return "the first word of its ID line has fewer than 7 fields between ':' (instrument:run:flowcell:lane:tile:x:y is expected)";
    case FQD_PLACE_EMPTY_FIELD: return "one of the first 7 fields of its ID line's first word is empty";
    case FQD_PLACE_NOT_DIGIT: return "its tile or x (fields 5 and 6) holds a byte that is no digit, or its y (field 7) does not begin with one";
    case FQD_PLACE_TOO_LONG: return "its tile, x or y has more than 9 digits";
    case FQD_PLACE_BAD_END: return "the digits of its y (field 7) are followed by something other than ':', '_', '#', '/' or the end of the ID line's first word";
    }
    return "its place on the flow cell was refused";
}

std::string sizein_reason(uint32_t reason)
{
    switch (reason) {
    case FQD_SIZEIN_NO_DIGITS: return "the `;size=` in the first word of its ID line is followed by no digit";
    case FQD_SIZEIN_BAD_END: return "the digits of its `;size=` are followed by something other than ';' or the end of the ID line's first word";
    case FQD_SIZEIN_ZERO: return "its annotation says `;size=0`: a record stands for at least one read";
    case FQD_SIZEIN_TOO_LARGE: return "its `;size=` has more than 10 digits or says more than 2147483647";
    case FQD_SIZEIN_TWICE: return "the first word of its ID line holds `;size=` twice";
    case FQD_SIZEIN_MATES_DIFFER: return "its `;size=` does not say what the record's annotation in file 1 says (1 where file 1 has none)";
    }
    return "its `;size=` annotation was refused";
}

} // namespace detail
} // namespace fqdhost
