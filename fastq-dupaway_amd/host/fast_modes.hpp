// fast_modes.hpp — the seventeen FQD_FAST_* switches of the `--fast` mode as one value: read from the environment in one place
// (FastModes::from_env), checked against the command line before any GPU call (check), and asked by the run
// (run_resident.cpp) through the predicates below.  Also the words of every refusal the switches can cause.
// Plain C++: no HIP, nothing of run_common.hpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "records.hpp"

namespace fqdhost {
namespace detail {

// Why a run with a switch set ends: the modes need every record's flag to stay open until the last record is in, or turn
// the reads where they lie in HBM, which only the GPU-resident ordered run offers (the streaming run's flags are final
// batch by batch).  Thrown before any output exists.
struct FastModeRefusal : std::runtime_error { using std::runtime_error::runtime_error; };

struct FastModes {
    bool keep_best = false;      // FQD_FAST_KEEP=first|best: a cluster's first member in the input is written, as in the reference, or the one with the best quality line (csrc/fqd_seq_pick_core.hpp)
    bool clusters = false;       // FQD_FAST_CLUSTERS=1: `<output>.clusters` beside every output
    bool both_strands = false;   // FQD_FAST_STRAND=given|both: both: a read and its reverse complement — a pair and the pair with its mates exchanged — are one key (csrc/fqd_strand_core.hpp)
    int umi = 0;                 // FQD_FAST_UMI=off|colon|underscore: 0, ':' or '_'; the UMI bases behind the last such byte of the first word of file 1's ID line are keyed in front of the sequence(s) (csrc/fqd_umi_core.hpp)
    int umi_mismatch = 0;        // FQD_FAST_UMI_MISMATCH=0|1|2: exact UMI clusters of one sequence (pair) whose UMIs differ in at most that many bases merge by UMI-tools' directional rule (csrc/fqd_umi_merge_core.hpp)
    bool size_out = false;       // FQD_FAST_SIZEOUT=1: every record written carries `;size=N`, its cluster's member count, behind the first word of its ID line (csrc/fqd_size_core.hpp)
    bool levels = false;         // FQD_FAST_LEVELS=1: `<output 1>.duplevels`, the clusters and records per duplication level
    bool sort_by_size = false;   // FQD_FAST_SORT=input|size: size: by decreasing cluster size, clusters of one size in the order of their first member (csrc/fqd_size_order_core.hpp)
    uint32_t min_size = 1, max_size = 0;   // FQD_FAST_MINSIZE=N / FQD_FAST_MAXSIZE=N in 1 .. 2^31-1: a cluster of fewer / more members is not written; unset: 1 and 0, the two that take nothing out
    bool size_in = false;        // FQD_FAST_SIZEIN=1: a `;size=N` an ID line already carries is the record's weight, a cluster's size the sum of its members' weights (csrc/fqd_sizein_core.hpp)
    uint32_t optical = 0;        // FQD_FAST_OPTICAL=D in 1 .. 2^31-1 (unset and 0: off): only the copies of a read within D pixels of each other on one tile of the flow cell, by the place in file 1's ID line, are duplicates (csrc/fqd_optical_core.hpp)
    uint32_t hamming = 0;        // FQD_FAST_HAMMING=D in 1 .. 3 (unset and 0: off): exact clusters of one shape whose sequences differ in at most D substituted bases a mate are one cluster, by single linkage; its first record is written (csrc/fqd_near_core.hpp)
    uint32_t umi_hamming = 0;    // FQD_FAST_UMI_HAMMING=D in 1 .. 3 (unset and 0: off; needs FQD_FAST_UMI): exact clusters under ONE UMI, of one shape, whose sequences differ in at most D substituted bases a mate are one molecule, by single linkage, together with FQD_FAST_UMI_MISMATCH's clusters; its first record is written (csrc/fqd_near_umi_core.hpp)
    bool centroid = false;       // FQD_FAST_CENTROID=first|abundant: abundant: a merged cluster is written by the first copy of its most abundant exact sequence (UMI and sequence), not by its first record (csrc/fqd_centroid_core.hpp)
    bool consensus = false;      // FQD_FAST_CONSENSUS=1: the sequence and quality lines of every cluster's written member are replaced by the cluster's column-wise consensus (csrc/fqd_consensus_core.hpp)
    bool longest = false;        // FQD_FAST_CENTROID=longest (the variable's third value; needs FQD_FAST_PREFIX): a merged cluster is written by the first copy of its root sequence, the one all its members are prefixes of
    uint32_t prefix = 0;         // FQD_FAST_PREFIX=L in 1 .. 65535 (unset and 0: off): an exact cluster whose reads are prefixes of another's, over at least L bases a mate, goes to the shortest such cluster; a tree of that relation is one cluster and its first record is written (csrc/fqd_prefix_core.hpp)

    // Reads the seventeen variables.  Throws std::runtime_error on a value that is none of the above, and FastModeRefusal for
    // a MAXSIZE below MINSIZE, in the order KEEP, SORT, MINSIZE, MAXSIZE, MAXSIZE below MINSIZE, STRAND, UMI, UMI_MISMATCH,
    // OPTICAL, HAMMING, UMI_HAMMING, CENTROID, PREFIX.  (CENTROID's words for a bad value name the two values it had first.)
    static FastModes from_env();
    // What the values and the command line decide, before any GPU call; throws FastModeRefusal.  In this order: SIZEIN with
    // nothing that reads sizes, UMI_MISMATCH without UMI, HAMMING with STRAND=both, HAMMING with UMI, UMI_HAMMING without UMI,
    // UMI_HAMMING with STRAND=both, CONSENSUS with STRAND=both, CONSENSUS with SIZEIN, CENTROID=abundant with no merging switch,
    // `--unordered`, several devices, KEEP=best with FASTA, CONSENSUS with FASTA, PREFIX with HAMMING, PREFIX with UMI (and so
    // with the two UMI merges), PREFIX with STRAND=both, PREFIX with CONSENSUS, CENTROID=longest without PREFIX.
    void check(bool unordered, size_t n_devices, Format format) const;

    bool size_filter() const { return min_size > 1 || max_size != 0; }                 // a bound that can take a cluster out
    bool sized() const { return size_out || levels || sort_by_size || size_filter(); } // something reads the cluster sizes
    bool linked() const { return keep_best || clusters || umi_mismatch || umi_hamming || optical || hamming || consensus || centroid || longest || prefix || sized(); }   // the duplicates must be linked to their clusters
    bool any() const { return linked() || both_strands || umi; }                       // only the GPU-resident ordered run will do

    // The switches that are set, as the messages name them: "FQD_FAST_KEEP=best and FQD_FAST_UMI=colon"; "" for none.
    std::string names() const;
    std::string umi_name() const { return umi == ':' ? "FQD_FAST_UMI=colon" : umi == '_' ? "FQD_FAST_UMI=underscore" : ""; }
    std::string mismatch_name() const { return umi_mismatch ? "FQD_FAST_UMI_MISMATCH=" + std::to_string(umi_mismatch) : std::string(); }
    std::string hamming_name() const { return hamming ? "FQD_FAST_HAMMING=" + std::to_string(hamming) : std::string(); }
    std::string umi_hamming_name() const { return umi_hamming ? "FQD_FAST_UMI_HAMMING=" + std::to_string(umi_hamming) : std::string(); }
    std::string prefix_name() const { return prefix ? "FQD_FAST_PREFIX=" + std::to_string(prefix) : std::string(); }
    bool merges() const { return umi_mismatch || hamming || umi_hamming || prefix; }     // a cluster may hold several exact sequences
    bool picks_centroid() const { return centroid || longest; }                          // another sequence than the first record's may be written: the exact owners stay
    std::string optical_name() const { return optical ? "FQD_FAST_OPTICAL=" + std::to_string(optical) : std::string(); }
    // What did not fit when the GPU-resident run meets the end of HBM, for the refusal.
    std::string out_of_memory_note() const;
};

// Why fqd_umi_find (enum fqd_umi_reason), fqd_size_annotations (enum fqd_sizein_reason) and fqd_read_places (enum
// fqd_place_reason) refuse a record, in the words of csrc/fqd_umi_core.hpp, csrc/fqd_sizein_core.hpp and csrc/fqd_optical_core.hpp.
std::string umi_reason(uint32_t reason, int sep);
std::string sizein_reason(uint32_t reason);
std::string optical_reason(uint32_t reason);

} // namespace detail
} // namespace fqdhost
