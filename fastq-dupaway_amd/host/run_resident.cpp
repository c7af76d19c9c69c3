// run_resident.cpp — the two runs whose text is resident in HBM, ordered (run_ordered_resident) and `--unordered`
// (run_unordered_resident); how the files get there is resident_input.cpp's.
#include "run_common.hpp"

namespace fqdhost {
using namespace detail;

namespace detail {

// FQD_FAST_KEEP=first|best: which member of a cluster of identical reads (pairs) `--fast` writes.  first (and unset): the
// first in the input, as the reference does; best: the one with the best quality line, at its own place in the input
// (csrc/fqd_owner_core.hpp, csrc/fqd_seq_pick_core.hpp).  Read here and nowhere else.
bool fast_keep_best()
{
    const char* v = std::getenv("FQD_FAST_KEEP");
    if (!v || std::strcmp(v, "first") == 0) return false;
    if (std::strcmp(v, "best") == 0) return true;
    throw std::runtime_error(std::string("FQD_FAST_KEEP must be 'first' or 'best', not '") + v + "'");
}

// FQD_FAST_CLUSTERS=1: `--fast` writes `<output>.clusters` beside every output.  Read here and nowhere else.
bool fast_clusters()
{
    const char* v = std::getenv("FQD_FAST_CLUSTERS");
    return v && std::atoi(v) != 0;
}

// FQD_FAST_STRAND=given|both: whether `--fast` tells the two strands of a fragment apart.  given (and unset): a read is
// what its bytes are, as in the reference; both: a read and its reverse complement — a pair and the pair with its mates
// exchanged — are one key (csrc/fqd_strand_core.hpp).  Read here and nowhere else.
bool fast_both_strands()
{
    const char* v = std::getenv("FQD_FAST_STRAND");
    if (!v || std::strcmp(v, "given") == 0) return false;
    if (std::strcmp(v, "both") == 0) return true;
    throw std::runtime_error(std::string("FQD_FAST_STRAND must be 'given' or 'both', not '") + v + "'");
}

// FQD_FAST_UMI=off|colon|underscore: whether `--fast` keys a read (pair) by the unique molecular identifier in file 1's ID
// lines as well.  off (and unset): by its sequence(s) alone; colon / underscore: by the UMI bases behind the last ':' / '_'
// of the ID line's first word, then the sequence(s) (csrc/fqd_umi_core.hpp).  Returns 0, ':' or '_'.  Read here and
// nowhere else.
int fast_umi()
{
    const char* v = std::getenv("FQD_FAST_UMI");
    if (!v || std::strcmp(v, "off") == 0) return 0;
    if (std::strcmp(v, "colon") == 0) return ':';
    if (std::strcmp(v, "underscore") == 0) return '_';
    throw std::runtime_error(std::string("FQD_FAST_UMI must be 'off', 'colon' or 'underscore', not '") + v + "'");
}

// FQD_FAST_UMI_MISMATCH=0|1|2: with FQD_FAST_UMI, whether the exact UMI clusters of one sequence (pair of sequences) whose UMIs
// differ in at most that many bases are merged by UMI-tools' directional rule (csrc/fqd_umi_merge_core.hpp).  0 (and unset):
// a UMI is told apart by every base.  Read here and nowhere else.
int fast_umi_mismatch()
{
    const char* v = std::getenv("FQD_FAST_UMI_MISMATCH");
    if (!v || std::strcmp(v, "0") == 0) return 0;
    if (std::strcmp(v, "1") == 0) return 1;
    if (std::strcmp(v, "2") == 0) return 2;
    throw std::runtime_error(std::string("FQD_FAST_UMI_MISMATCH must be 0, 1 or 2, not '") + v + "'");
}

// FQD_FAST_SIZEOUT=1: every record `--fast` writes carries `;size=N`, its cluster's member count, behind the first word of
// its ID line (csrc/fqd_size_core.hpp).  Read here and nowhere else.
bool fast_sizeout()
{
    const char* v = std::getenv("FQD_FAST_SIZEOUT");
    return v && std::atoi(v) != 0;
}

// FQD_FAST_LEVELS=1: `--fast` writes `<output 1>.duplevels`, the clusters and records per duplication level.  Read here and
// nowhere else.
bool fast_levels()
{
    const char* v = std::getenv("FQD_FAST_LEVELS");
    return v && std::atoi(v) != 0;
}

// FQD_FAST_SORT=input|size: the order of the records `--fast` writes.  input (and unset): the input's; size: by decreasing
// cluster size, clusters of one size in the order of their first member (csrc/fqd_size_order_core.hpp).  Read here and
// nowhere else.
bool fast_sort_by_size()
{
    const char* v = std::getenv("FQD_FAST_SORT");
    if (!v || std::strcmp(v, "input") == 0) return false;
    if (std::strcmp(v, "size") == 0) return true;
    throw std::runtime_error(std::string("FQD_FAST_SORT must be 'input' or 'size', not '") + v + "'");
}

// FQD_FAST_MINSIZE=N / FQD_FAST_MAXSIZE=N: a cluster of fewer / more members than N is not written.  `unset` where the
// variable is not set (1 and 0, "no bound").  Read here and nowhere else.
uint32_t fast_size_bound(const char* name, uint32_t unset)
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

// FQD_FAST_SIZEIN=1: a `;size=N` that the first word of an ID line already carries is the record's weight, a cluster's size
// is the sum of its members' weights, and with FQD_FAST_SIZEOUT the new label takes the old annotation's place
// (csrc/fqd_sizein_core.hpp).  Read here and nowhere else.
bool fast_sizein()
{
    const char* v = std::getenv("FQD_FAST_SIZEIN");
    return v && std::atoi(v) != 0;
}

} // namespace detail

namespace {

// Why a run with FQD_FAST_KEEP=best or FQD_FAST_CLUSTERS=1 ends: these modes need every record's flag to stay open until
// the last record is in, which only the GPU-resident run offers (the streaming run's flags are final batch by batch).
// FQD_FAST_STRAND=both ends the same way: it turns the reads where they lie in HBM, in front of the engine.
struct FastModeRefusal : std::runtime_error { using std::runtime_error::runtime_error; };

const char* umi_switch(int umi) { return umi == ':' ? "FQD_FAST_UMI=colon" : umi == '_' ? "FQD_FAST_UMI=underscore" : nullptr; }

const char* mismatch_switch(int mismatch) { return mismatch == 1 ? "FQD_FAST_UMI_MISMATCH=1" : mismatch == 2 ? "FQD_FAST_UMI_MISMATCH=2" : nullptr; }

// (min_size 1 and max_size 0 are the two bounds that take nothing out: not named)
std::string fast_switches(bool best, bool clusters, bool both, int umi, int mismatch, bool sizeout, bool levels, bool by_size, uint32_t min_size, uint32_t max_size,
                          bool sizein)
{
    std::string s;
    for (const char* name : {best ? "FQD_FAST_KEEP=best" : nullptr, clusters ? "FQD_FAST_CLUSTERS=1" : nullptr, both ? "FQD_FAST_STRAND=both" : nullptr, umi_switch(umi),
                             mismatch_switch(mismatch), sizeout ? "FQD_FAST_SIZEOUT=1" : nullptr, levels ? "FQD_FAST_LEVELS=1" : nullptr,
                             by_size ? "FQD_FAST_SORT=size" : nullptr, sizein ? "FQD_FAST_SIZEIN=1" : nullptr})
        if (name) s += (s.empty() ? "" : " and ") + std::string(name);
    if (min_size > 1) s += (s.empty() ? "" : " and ") + ("FQD_FAST_MINSIZE=" + std::to_string(min_size));
    if (max_size) s += (s.empty() ? "" : " and ") + ("FQD_FAST_MAXSIZE=" + std::to_string(max_size));
    return s;
}

// Why fqd_umi_find refuses a record (enum fqd_umi_reason), in the words of csrc/fqd_umi_core.hpp.
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

// Why fqd_size_annotations refuses a record (enum fqd_sizein_reason), in the words of csrc/fqd_sizein_core.hpp.
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

} // namespace

// Everything about the eleven switches that their values and the command line decide, before any GPU call.
void HashDupRemover::read_fast_modes(bool unordered)
{
    sort_by_size_ = fast_sort_by_size();
    min_size_ = fast_size_bound("FQD_FAST_MINSIZE", 1);
    max_size_ = fast_size_bound("FQD_FAST_MAXSIZE", 0);
    if (max_size_ && max_size_ < min_size_)
        throw FastModeRefusal("FQD_FAST_MAXSIZE=" + std::to_string(max_size_) + " is below FQD_FAST_MINSIZE=" + std::to_string(min_size_) + ": no cluster could be written");
    size_filter_ = min_size_ > 1 || max_size_ != 0;
    keep_best_ = fast_keep_best();
    write_clusters_ = fast_clusters();
    both_strands_ = fast_both_strands();
    umi_sep_ = fast_umi();
    umi_mismatch_ = fast_umi_mismatch();
    size_out_ = fast_sizeout();
    write_levels_ = fast_levels();
    size_in_ = fast_sizein();
    if (size_in_ && !size_out_ && !write_levels_ && !sort_by_size_ && !size_filter_)
        throw FastModeRefusal("FQD_FAST_SIZEIN=1 changes what a cluster's size is and nothing else: set one of FQD_FAST_SIZEOUT=1, FQD_FAST_LEVELS=1, FQD_FAST_SORT=size, "
                              "FQD_FAST_MINSIZE (above 1) or FQD_FAST_MAXSIZE as well, which read the sizes");
    if (!keep_best_ && !write_clusters_ && !both_strands_ && !umi_sep_ && !umi_mismatch_ && !size_out_ && !write_levels_ && !sort_by_size_ && !size_filter_) return;
    const std::string which = fast_switches(keep_best_, write_clusters_, both_strands_, umi_sep_, umi_mismatch_, size_out_, write_levels_, sort_by_size_, min_size_, max_size_, size_in_);
    if (umi_mismatch_ && !umi_sep_)
        throw FastModeRefusal(std::string(mismatch_switch(umi_mismatch_)) + " merges the UMIs that FQD_FAST_UMI finds: set FQD_FAST_UMI=colon or FQD_FAST_UMI=underscore as well");
    if (unordered)
        throw FastModeRefusal(which + " with --unordered: these modes run on ordered inputs only");
    if (tuning_.devices.size() > 1)
        throw FastModeRefusal(which + " runs on one GPU: FQD_DEVICES may name one device only");
    if (keep_best_ && format_ == Format::Fasta)
        throw FastModeRefusal("FQD_FAST_KEEP=best needs the quality lines of FASTQ records: --format fasta has none");
    if (tuning_.devices.size() == 1) { tuning_.device = tuning_.devices[0]; tuning_.devices.clear(); }
}

// An ordered run (single-end, or paired files read side by side) with a codec at either end — BGZF inputs, or `.gz`
// outputs of plain regular inputs: the files go to HBM as they lie on disk, are inflated (if compressed) and cut into
// records there, every read (pair) is deduplicated where it lies, and the
// survivors leave in input order window by window (deflated on the device for `.gz` outputs).  Taken only when
// everything is plain sailing — regular BGZF files of whole records, as many in file 2 as in file 1, no unknown
// base, everything fits in HBM; otherwise false is returned BEFORE any output is touched and the streaming run
// (run_ordered), which reproduces the reference's behaviour for every irregular input, does the job.
//
// With FQD_FAST_KEEP=best or FQD_FAST_CLUSTERS=1 (`modes`) the run is taken for plain files as well, links every duplicate
// to an earlier record of its key (fqd_submit_linked), resolves the links to the first record (fqd_owners), groups the
// records by it (fqd_group_owners) and, for `best`, moves the keep flag of every cluster to its best member
// (pick_best_members, fqd_heads_to_keep).  There is no hand-over then: whatever would have sent the input to the
// streaming run ends the run with a message that names the switch and the reason, still before any output exists.
//
// With FQD_FAST_STRAND=both (also `modes`) one fqd_canonical_reads over all n records stands between the record scan and
// the submit loop, which then submits the canonical descriptors; whatever comes after the loop sees flags and links as
// before, and the writers take the records' ORIGINAL text.
//
// With FQD_FAST_UMI=colon|underscore (also `modes`) one more rewrite stands at that place, behind the strand block:
// fqd_umi_find over file 1's ID lines — a record it refuses ends the run — then fqd_umi_reads, which packs `UMI bases ‖
// sequence` of mate 1 (the canonical mate 1 with FQD_FAST_STRAND=both) for the submit loop's segment 0.  Mate 2 goes to the
// submit as it is.
//
// With FQD_FAST_SIZEOUT=1 or FQD_FAST_LEVELS=1 (both `linked`) one fqd_cluster_sizes follows the grouping and the pick: the
// member count of every cluster at the record that is written, 4 bytes a record, and the level table.  The table becomes
// `<output 1>.duplevels`; the sizes stay for the writer when FQD_FAST_SIZEOUT is set, which then plans the outputs from the
// records' sizes with their labels and copies the windows with fqd_copy_labelled (survivor_writer.cpp), and are released
// at once otherwise.
//
// With FQD_FAST_SORT=size, FQD_FAST_MINSIZE or FQD_FAST_MAXSIZE (all `linked`) the sizes are computed as well, while perm and
// head still exist: fqd_size_filter clears the flags of the clusters outside the bounds — behind the cluster files and the
// level table, which hold all clusters — and fqd_size_order writes the records that stay in order of decreasing cluster
// size.  The writer then takes that order as its index for both files, a set flag for each of its entries, and as many
// pairs as it has entries; with FQD_FAST_SIZEOUT the labels are still found per record and brought into the order by
// fqd_take_u32 (survivor_writer.cpp).  A filter without the order needs no index: the cleared flags go through the plan.
//
// With FQD_FAST_SIZEIN=1 (beside at least one of the five size switches) fqd_size_annotations reads every record's weight off
// its ID line where fqd_umi_find runs, before the first submit — file 1 gives the weights, file 2 is held against them, and a
// record it refuses ends the run —, fqd_cluster_weights stands wherever fqd_cluster_sizes would, and the weights are released
// after the last such call.  Everything that reads sizes reads the weighted ones; the writer parses the annotations' places
// once more per file (survivor_writer.cpp), so nothing but the weights is held in between.
//
// With FQD_FAST_UMI_MISMATCH=1|2 (also `linked`; FQD_FAST_UMI is set) the engine is used TWICE: the submit loop as above
// keyed `UMI bases ‖ sequence` gives the exact owners and, through fqd_group_owners and fqd_cluster_sizes, every exact
// cluster's count; after fqd_engine_reset the same batches go in again keyed by the sequences alone (the given or the
// canonical descriptors), into the same flags and links, which gives every record's sequence group.  fqd_umi_merge makes
// the merged owners of the three, fqd_owners_to_keep the flags, and the grouping, the pick, the cluster files, the sizes
// and the writers follow as they do for any other owners.  The canonical and keyed buffers stay until the second pass is
// through, the UMI offsets until the merge is.
bool HashDupRemover::run_ordered_resident(int S, const std::string* in, const std::string* out)
{
    const bool linked = keep_best_ || write_clusters_ || size_out_ || write_levels_ || umi_mismatch_ || sort_by_size_ || size_filter_, modes = linked || both_strands_ || umi_sep_;
    const std::string which = fast_switches(keep_best_, write_clusters_, both_strands_, umi_sep_, umi_mismatch_, size_out_, write_levels_, sort_by_size_, min_size_, max_size_, size_in_);
    // FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE: what `-v` says behind its first line
    auto print_not_written = [&](uint64_t clusters, uint64_t records) {
        if (verbose_ && size_filter_)
            std::cout << clusters << " clusters holding " << records << (S == 1 ? " reads" : " read pairs") << " were not written (FQD_FAST_MINSIZE=" << min_size_
                      << ", FQD_FAST_MAXSIZE=" << (max_size_ ? std::to_string(max_size_) : std::string("none")) << ").\n";
    };
    auto give_up = [&](const std::string& why) -> bool {
        if (modes) throw FastModeRefusal(which + ": the GPU-resident run cannot take this input (" + why +
                                         "), and the streaming run cannot serve these modes");
        return false;
    };
    // (both are decided before any GPU call)
    if (const char* v = std::getenv("FQD_ORDERED_RESIDENT")) if (std::atoi(v) == 0) return give_up("FQD_ORDERED_RESIDENT=0 turns that run off");
    if (!inflate_on_device()) {
        bool gz = !modes;                                         // with a switch set only a `.gz` input needs the device inflate
        for (int s = 0; s < S; ++s) gz |= has_gz_extension(in[s]);
        if (gz) return give_up("FQD_GUNZIP_DEVICE=0 keeps `.gz` inputs off the GPU");
    }
    // worth it when a codec is involved: a BGZF input, or a `.gz` output the GPU can deflate (plain files in and
    // out are better off in the streaming run, where reading, the GPU and writing overlap)
    bool any_gz_in = false, any_gz_out = false, all_empty = true;
    for (int s = 0; s < S; ++s) {
        uint64_t size = 0;
        if (!is_regular_file(in[s], size)) return give_up(in[s] + " is not a regular file: a pipe cannot be held in GPU memory");
        all_empty &= size == 0;
        any_gz_in |= has_gz_extension(in[s]);
        any_gz_out |= has_gz_extension(out[s]);
    }
    if (!modes && !any_gz_in && !(any_gz_out && deflate_on_device())) return false;
    if (modes && all_empty) {
        // no record, no cluster, nothing to choose: what the default run makes of empty files, and empty cluster files
        // (the table of zeros is written whatever the default run makes of an empty file, behind its outputs)
        struct LevelsOfNothing { bool on; const std::string& name; ~LevelsOfNothing() { if (on) write_cluster_lines(duplevels_text(fqd_size_levels{}), name + ".duplevels"); } }
            levels_of_nothing{write_levels_, out[0]};
        run_ordered(S, in, out);                                  // (no cluster, no filter: the second `-v` line is not said either)
        if (write_clusters_) for (int s = 0; s < S; ++s) write_cluster_lines(std::string(), out[s] + ".clusters");
        return true;
    }
    HIP_OK(hipSetDevice(tuning_.device));
    StreamGuard stream;
    const size_t fetch_bytes = fetch_bytes_for(block_bytes_for(tuning_, memlimit_), memlimit_);
    FileOnDevice dev[2];
    Device<uint8_t> keep;
    Device<uint32_t> link, owner, perm; Device<uint8_t> head;     // FQD_FAST_KEEP / FQD_FAST_CLUSTERS / FQD_FAST_SIZEOUT / FQD_FAST_LEVELS
    Device<uint32_t> cluster_size; fqd_size_levels levels{};      // FQD_FAST_SIZEOUT / FQD_FAST_LEVELS / FQD_FAST_SORT / FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE
    Device<uint32_t> order; Device<uint8_t> all_kept;             // FQD_FAST_SORT=size: the written order and a set flag for each of its entries
    uint64_t n_written = 0, dropped_clusters = 0, dropped_records = 0;
    Device<uint8_t> canon, turned; Device<uint64_t> canon_off[2]; Device<uint32_t> canon_len[2];   // FQD_FAST_STRAND=both
    Device<uint8_t> umi_text; Device<uint64_t> umi_off64; Device<uint32_t> umi_len, umi_off;        // FQD_FAST_UMI
    Device<uint32_t> owner_seq, exact_size, merged_owner;        // FQD_FAST_UMI_MISMATCH
    Device<uint32_t> weight;                                     // FQD_FAST_SIZEIN: what every record stands for, while sizes are made
    fqd_umi_info umi_info{};
    uint32_t umi_bases = 0;
    std::string clusters[2];
    uint64_t n = 0, dups = 0;
    std::unique_ptr<EngineHandle> eng;
    SurvivorBuffers buffers;
    std::thread make_engine; std::exception_ptr engine_error;
    struct JoinGuard { std::thread& t; ~JoinGuard() { if (t.joinable()) t.join(); } } join_guard{make_engine};
    try {
        Fetched got[2];                                            // (way None: not fetched, an exception included)
        bool no_room[2] = {false, false};
        std::exception_ptr fetch_error[2];
        // the engine — its key store and table sized from the files' sizes — is made on a helper thread under the reads
        uint64_t cap_reads = 0, cap_bases = 0;
        guess_capacity(S, in, cap_reads, cap_bases);
        make_engine = std::thread([&] {
            try { HIP_OK(hipSetDevice(tuning_.device)); StageClock::Scope t("  on the GPU: engine, key store, table (under the read)"); eng = std::make_unique<EngineHandle>(S, tuning_.device, stream, cap_reads, cap_bases); }
            catch (...) { engine_error = std::current_exception(); }
        });
        {
            StageClock::Scope t("ordered/resident: files to HBM");
            auto fetch = [&](int s) {
                try { fetch_file(in[s], fetch_bytes, tuning_.device, dev[s], got[s]); }
                catch (const DeviceOutOfMemory&) { no_room[s] = true; }
                catch (const DeviceError&) { fetch_error[s] = std::current_exception(); }
                catch (const std::exception&) {}                           // the host reader will say what is wrong with the file
            };
            std::thread second;
            if (S == 2) second = std::thread(fetch, 1);
            fetch(0);
            if (S == 2) second.join();
        }
        if (make_engine.joinable()) make_engine.join();
        for (int s = 0; s < S; ++s) if (fetch_error[s]) std::rethrow_exception(fetch_error[s]);
        for (int s = 0; s < S; ++s)
            if (got[s].way == Fetched::None) return give_up(no_room[s] ? in[s] + " does not fit in GPU memory" : in[s] + " could not be taken to GPU memory as it lies on disk (empty, damaged, or changed while it was read)");
        if (engine_error) std::rethrow_exception(engine_error);
        {
            StageClock::Scope t("ordered/resident: inflate + record scan on the GPU");
            for (int s = 0; s < S; ++s)
                if (!cut_records(eng->e, stream, format_, got[s], dev[s])) return give_up(in[s] + " does not hold whole, well-formed records");
        }
        if (S == 2 && dev[0].n != dev[1].n) return give_up("the two files hold different numbers of records");
        n = dev[0].n;
        if (linked && n >= 0x80000000ull)
            throw FastModeRefusal(which + ": at most 2^31-1 records (pairs) per run, the input holds " + std::to_string(n));
        if ((both_strands_ || umi_sep_) && n > 0xFFFFFFFEull)
            throw FastModeRefusal(which + ": at most 2^32-2 records (pairs) per run, the input holds " + std::to_string(n));
        StageClock::Scope t("ordered/resident: dedup on the GPU");
        keep.reserve(n);
        if (linked) { link.reserve(n); owner.reserve(n); perm.reserve(n); head.reserve(n); }
        if (umi_mismatch_) { owner_seq.reserve(n); exact_size.reserve(n); merged_owner.reserve(n); }
        // no more than a file's sequence bytes — a FASTQ record is its sequence twice (bases, qualities) and at least six
        // more bytes, a FASTA record its sequence and at least three
        auto seq_bound = [&](int s) -> uint64_t {
            return format_ == Format::Fasta ? dev[s].text.used - std::min<uint64_t>(dev[s].text.used, 3 * n)
                                            : (dev[s].text.used - std::min<uint64_t>(dev[s].text.used, 6 * n)) / 2 + 1;
        };
        fqd_reads given[2] = {};
        for (int s = 0; s < S; ++s) {
            given[s].bases = reinterpret_cast<const uint8_t*>(dev[s].text.p);
            given[s].offsets = dev[s].seq_off.p; given[s].lengths = dev[s].seq_len.p;
        }
        if (both_strands_) {
            // the canonical sequences and their descriptors
            uint64_t bound = 0;
            for (int s = 0; s < S; ++s) bound += seq_bound(s);
            canon.reserve(bound + 64); turned.reserve(n);
            for (int s = 0; s < S; ++s) { canon_off[s].reserve(n); canon_len[s].reserve(n); }
            StageClock::Scope t2("fast: both strands, canonical reads on the GPU");
            uint64_t n_turned = 0;
            engine_ok<DeviceError>(eng->e, fqd_canonical_reads(eng->e, given, n, canon.p, bound, canon_off[0].p, canon_len[0].p,
                                                               S == 2 ? canon_off[1].p : nullptr, S == 2 ? canon_len[1].p : nullptr, turned.p,
                                                               StageClock::on() ? &n_turned : nullptr));
            if (StageClock::on()) std::cerr << "fast: both strands, " << n_turned << " of " << n << " records turned\n";
        }
        if (umi_sep_) {
            StageClock::Scope t2("fast: UMI, find and pack on the GPU");
            const uint8_t* text0 = reinterpret_cast<const uint8_t*>(dev[0].text.p);
            umi_off.reserve(n);
            fqd_umi_info& info = umi_info;
            engine_ok<DeviceError>(eng->e, fqd_umi_find(eng->e, text0, dev[0].start.p, dev[0].id_len.p, n, umi_sep_, umi_off.p, &info));
            if (info.bad_record != FQD_UMI_NO_RECORD)
                throw FastModeRefusal(std::string(umi_switch(umi_sep_)) + ": record " + std::to_string(info.bad_record) + " (counted from 0) of " + in[0] +
                                      ": " + umi_reason(info.bad_reason, umi_sep_));
            umi_bases = info.n_bases;
            // mate 1's sequence bytes (with both strands the canonical mate 1 of a pair may be either file's read), the UMI
            // bases of every record, and the descriptors
            const uint64_t bound = seq_bound(0) + (both_strands_ && S == 2 ? seq_bound(1) : 0) + uint64_t(umi_bases) * n;
            umi_text.reserve(bound + 64); umi_off64.reserve(n); umi_len.reserve(n);
            const fqd_reads mate0 = both_strands_ ? fqd_reads{canon.p, canon_off[0].p, canon_len[0].p, 0, 0} : given[0];
            engine_ok<DeviceError>(eng->e, fqd_umi_reads(eng->e, text0, dev[0].start.p, umi_off.p, &info, &mate0, n, umi_text.p, bound, umi_off64.p, umi_len.p));
            if (StageClock::on()) std::cerr << "fast: UMI, " << umi_bases << " bases behind the last '" << char(umi_sep_) << "' of the first word\n";
        }
        if (size_in_) {
            // the weights, before anything else is spent on an input with a malformed annotation
            StageClock::Scope t2("fast: size annotations on the GPU");
            weight.reserve(n);
            fqd_sizein_info info{};
            for (int s = 0; s < S; ++s) {
                fqd_sizein_info found{};
                engine_ok<DeviceError>(eng->e, fqd_size_annotations(eng->e, reinterpret_cast<const uint8_t*>(dev[s].text.p), dev[s].start.p, dev[s].id_len.p, n,
                                                                    s ? weight.p : nullptr, s ? nullptr : weight.p, nullptr, nullptr, &found));
                if (found.bad_record != FQD_UMI_NO_RECORD)
                    throw FastModeRefusal("FQD_FAST_SIZEIN=1: record " + std::to_string(found.bad_record) + " (counted from 0) of " + in[s] + ": " + sizein_reason(found.bad_reason));
                if (s == 0) info = found;
            }
            if (StageClock::on()) std::cerr << "fast: size annotations, " << info.annotated << " of " << n << " records annotated, total weight " << info.total_weight << "\n";
        }
        // fqd_cluster_sizes, or with FQD_FAST_SIZEIN the weighted sizes: a cluster above 2^31-1 ends the run
        auto cluster_sizes = [&](uint32_t* size, fqd_size_levels* lv) {
            if (!size_in_) { engine_ok<DeviceError>(eng->e, fqd_cluster_sizes(eng->e, perm.p, head.p, n, size, lv)); return; }
            fqd_weights_info over{};
            engine_ok<DeviceError>(eng->e, fqd_cluster_weights(eng->e, perm.p, head.p, weight.p, n, size, lv, &over));
            if (over.over_record != FQD_UMI_NO_RECORD)
                throw FastModeRefusal("FQD_FAST_SIZEIN=1: the cluster of record " + std::to_string(over.over_record) + " (counted from 0) of " + in[0] + " has the weighted size " +
                                      std::to_string(over.over_sum) + ": at most 2147483647");
        };
        // all n records through the engine, batch by batch; with_umi: mate 1 as `UMI bases ‖ sequence`
        auto submit_all = [&](bool with_umi) -> int {
            const size_t kBatch = 16u << 20;
            int rc = FQD_OK;
            for (size_t a = 0; a < n && rc == FQD_OK; a += kBatch) {
                fqd_reads seg[2] = {};
                for (int s = 0; s < S; ++s) {
                    seg[s].bases = both_strands_ ? canon.p : reinterpret_cast<const uint8_t*>(dev[s].text.p);
                    seg[s].offsets = (both_strands_ ? canon_off[s].p : dev[s].seq_off.p) + a;
                    seg[s].lengths = (both_strands_ ? canon_len[s].p : dev[s].seq_len.p) + a;
                }
                if (with_umi) seg[0] = fqd_reads{umi_text.p, umi_off64.p + a, umi_len.p + a, 0, 0};
                if (linked) rc = fqd_submit_linked(eng->e, seg, std::min<size_t>(kBatch, n - a), FQD_MEM_DEVICE, keep.p + a, link.p + a, a + kBatch < n ? 0 : 1);
                else rc = (a + kBatch < n ? fqd_submit : fqd_submit_final)(eng->e, seg, std::min<size_t>(kBatch, n - a), FQD_MEM_DEVICE, keep.p + a);
            }
            if (rc == FQD_OK) rc = fqd_engine_sync(eng->e);
            return rc;
        };
        int rc = submit_all(umi_sep_ != 0);
        if (rc == FQD_ERR_BAD_BASE)                              // the streaming run cuts the output where the reference does
            return give_up(std::string(fqd_last_error(eng->e)) + (umi_sep_ ? "; a position in mate 1 counts the " + std::to_string(umi_bases) + " UMI bases in front of the sequence" : std::string()));
        if (rc != FQD_OK) throw DeviceError(std::string("GPU engine: ") + fqd_last_error(eng->e));
        fqd_umi_merge_info merged{};
        if (umi_mismatch_) {
            // the exact owners and counts, then the same records once more without their UMIs: the flags and links of the
            // first pass are used up by fqd_owners and taken again
            uint64_t exact_clusters = 0;
            {
                StageClock::Scope t2("fast: UMI mismatches, exact owners and counts on the GPU");
                engine_ok<DeviceError>(eng->e, fqd_owners(eng->e, keep.p, link.p, n, owner.p));
                engine_ok<DeviceError>(eng->e, fqd_group_owners(eng->e, owner.p, n, perm.p, head.p, &exact_clusters));
                cluster_sizes(exact_size.p, nullptr);
            }
            {
                StageClock::Scope t2("fast: UMI mismatches, second pass by sequence on the GPU");
                engine_ok<DeviceError>(eng->e, fqd_engine_reset(eng->e));
                if (submit_all(false) != FQD_OK) throw DeviceError(std::string("GPU engine: ") + fqd_last_error(eng->e));
                engine_ok<DeviceError>(eng->e, fqd_owners(eng->e, keep.p, link.p, n, owner_seq.p));
            }
            StageClock::Scope t2("fast: UMI mismatches, networks on the GPU");
            engine_ok<DeviceError>(eng->e, fqd_umi_merge(eng->e, reinterpret_cast<const uint8_t*>(dev[0].text.p), dev[0].start.p, umi_off.p, &umi_info, owner.p,
                                                         owner_seq.p, exact_size.p, n, uint32_t(umi_mismatch_), merged_owner.p, &merged));
            if (merged.over_limit_first != FQD_UMI_NO_RECORD)
                throw FastModeRefusal(std::string(mismatch_switch(umi_mismatch_)) + ": the sequence of record " + std::to_string(merged.over_limit_first) + " (counted from 0) of " + in[0] +
                                      " stands under " + std::to_string(merged.over_limit_nodes) + " different UMIs, a network of at most " + std::to_string(merged.max_group) +
                                      " is merged (amplicon-style data: deduplicate it by exact UMI, without the switch)");
            if (merged.nodes != exact_clusters) throw DeviceError("GPU engine: internal error (the merge and the grouping count different exact clusters)");
            engine_ok<DeviceError>(eng->e, fqd_owners_to_keep(eng->e, merged_owner.p, n, keep.p));
            if (StageClock::on())
                std::cerr << "fast: UMI mismatches <= " << umi_mismatch_ << ", " << merged.merged << " of " << merged.nodes << " exact clusters merged into others, largest network "
                          << merged.largest << ", " << merged.sweeps << " sweeps\n";
            owner_seq.release(); exact_size.release();
        }
        canon.release(); turned.release();                       // the last submit is through: nothing below reads a turned byte
        for (int s = 0; s < 2; ++s) { canon_off[s].release(); canon_len[s].release(); }
        umi_text.release(); umi_off64.release(); umi_len.release(); umi_off.release();
        if (std::getenv("FQD_TEST_FAIL_RESIDENT")) throw DeviceError("GPU engine: forced by FQD_TEST_FAIL_RESIDENT");      // tests: the hand-over is announced
        fqd_stats st{};
        fqd_get_stats(eng->e, &st);
        dups = umi_mismatch_ ? n - (merged.nodes - merged.merged) : st.duplicates;
        FileOnDevice* all_files[2] = {&dev[0], &dev[1]};
        if (linked) {
            uint64_t n_clusters = 0;
            {
                StageClock::Scope t2("fast: owners and clusters on the GPU");
                if (!umi_mismatch_) engine_ok<DeviceError>(eng->e, fqd_owners(eng->e, keep.p, link.p, n, owner.p));
                engine_ok<DeviceError>(eng->e, fqd_group_owners(eng->e, umi_mismatch_ ? merged_owner.p : owner.p, n, perm.p, head.p, &n_clusters));
            }
            if (n_clusters + dups != n) throw DeviceError("GPU engine: internal error (the clusters and the duplicates do not add up to the records)");
            link.release(); owner.release(); merged_owner.release();
            if (keep_best_) {
                const uint64_t moved = pick_best_members(eng->e, S, all_files, n, head.p, perm.p, "fast: best-quality pick on the GPU");
                engine_ok<DeviceError>(eng->e, fqd_heads_to_keep(eng->e, perm.p, head.p, n, keep.p));
                if (StageClock::on()) std::cerr << "fast: best-quality pick, " << moved << " of " << n_clusters << " clusters changed\n";
            }
            if (write_clusters_) {
                StageClock::Scope t2("fast: ID lines of the clusters out of HBM");
                for (int s = 0; s < S; ++s) clusters[s] = cluster_lines(eng->e, stream, dev[s], perm.p, head.p, n);
            }
            if (size_out_ || write_levels_ || sort_by_size_ || size_filter_) {
                StageClock::Scope t2("fast: cluster sizes on the GPU");
                cluster_size.reserve(n);
                cluster_sizes(cluster_size.p, &levels);
                weight.release();
                if (StageClock::on()) std::cerr << "fast: cluster sizes, " << n_clusters << " clusters, largest " << levels.largest << "\n";
            }
            if (size_filter_) {
                // the clusters outside the bounds leave the flags; the cluster files and the level table have been made of all
                StageClock::Scope t2("fast: size filter on the GPU");
                engine_ok<DeviceError>(eng->e, fqd_size_filter(eng->e, cluster_size.p, n, min_size_, max_size_, keep.p, &dropped_clusters, &dropped_records));
                if (StageClock::on()) std::cerr << "fast: size filter, " << dropped_clusters << " clusters of " << dropped_records << " records not written\n";
            }
            n_written = n_clusters - dropped_clusters;
            if (sort_by_size_) {
                order.reserve(std::max<uint64_t>(n_written, 1)); all_kept.reserve(std::max<uint64_t>(n_written, 1));    // (a filter may leave nothing)
                uint64_t w = 0;
                fqd_size_order_info sorted{};
                {
                    StageClock::Scope t2("fast: abundance order on the GPU");
                    engine_ok<DeviceError>(eng->e, fqd_size_order_ex(eng->e, perm.p, head.p, cluster_size.p, keep.p, n, order.p, &w, &sorted));
                    if (w != n_written) throw DeviceError("GPU engine: internal error (the written order and the kept clusters differ in number)");
                    if (w) HIP_OK(hipMemsetAsync(all_kept.p, 1, w, stream));
                    HIP_OK(hipStreamSynchronize(stream));
                }
                // (what the call counted: the pairs of tier 1's bucket 0, which alone went through tier 2's passes)
                if (StageClock::on())
                    std::cerr << "fast: abundance order, " << w << " clusters written, " << sorted.large << " of them above 255 members sorted apart\n";
            }
            if (!size_out_) cluster_size.release();
            perm.release(); head.release();
        }
        // everything the writer needs is reserved HERE, while the run can still hand over: once an output exists it cannot
        bool gz_out[2] = {false, false};
        for (int s = 0; s < S; ++s) gz_out[s] = has_gz_extension(out[s]);
        FileOnDevice* files[2] = {&dev[0], &dev[1]};
        if (size_out_) { buffers.cluster_size = cluster_size.p; buffers.size_in = size_in_; }
        if (sort_by_size_) {
            // pair k is record order[k], of both files; every pair is written
            const uint32_t* idx[2] = {order.p, order.p};
            buffers.record_keep = keep.p; buffers.records = n;
            plan_survivors(eng->e, S, files, idx, all_kept.p, n_written, gz_out, memlimit_, buffers);
            cluster_size.release();                               // (the writer has the sizes in written order)
        } else {
            const uint32_t* idx[2] = {nullptr, nullptr};
            plan_survivors(eng->e, S, files, idx, keep.p, n, gz_out, memlimit_, buffers);
        }
    } catch (const FastModeRefusal&) {
        throw;                                                    // nothing has been written
    } catch (const DeviceOutOfMemory&) {
        // (what the two size switches and the mismatch switch add, named only when one of them is set)
        const bool sized = size_out_ || write_levels_ || sort_by_size_ || size_filter_;
        const std::string sizes = (!sized ? std::string() :
            std::string("; the cluster sizes of ") + (size_out_ ? "FQD_FAST_SIZEOUT" : write_levels_ ? "FQD_FAST_LEVELS" : sort_by_size_ ? "FQD_FAST_SORT" : "FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE") +
            " take 4 bytes a record more" +
            (size_out_ ? " and the labels' places and grown sizes 8 bytes a record and file" : "") +
            (size_in_ ? std::string("; FQD_FAST_SIZEIN takes 4 bytes a record for the weights while the sizes are made") +
                        (size_out_ ? " and 4 bytes a record and file for the annotations' lengths in the writer" : "") : std::string())) +
            (!sort_by_size_ ? std::string() : std::string("; FQD_FAST_SORT=size takes 4 bytes a cluster for the written order, 1 byte a cluster for its flags and, while it sorts, "
                                                          "24 bytes a cluster of scratch (the scratch of the grouping serves where it is as large)") +
                                              (size_out_ ? ", and the labels' places and the sizes in written order 4 bytes a cluster and file and 4 bytes a cluster" : "")) +
            (!umi_mismatch_ ? std::string() : std::string("; FQD_FAST_UMI_MISMATCH takes 12 bytes a record more (the owners by sequence, the exact counts, the merged owners) "
                                                          "and, while it merges, 4 bytes a record and up to 66 bytes an exact cluster"));
        if (umi_sep_)
            return give_up(std::string("the text, the record arrays, the keyed bytes of FQD_FAST_UMI (mate 1's sequence bytes once more and the UMI bases of every record, 16 bytes a record)") +
                           (both_strands_ ? ", the canonical reads (the sequence bytes once more, 12 bytes a record and mate, 1 byte a record)" : "") +
                           " and, with FQD_FAST_KEEP / FQD_FAST_CLUSTERS, up to 37 bytes a record for the links, the owners and their grouping do not fit in GPU memory" + sizes);
        return give_up((both_strands_ ? "the text, the record arrays, the canonical reads (the sequence bytes once more, 12 bytes a record and mate, 1 byte a record) and, with FQD_FAST_KEEP / FQD_FAST_CLUSTERS, up to 37 bytes a record for the links, the owners and their grouping do not fit in GPU memory"
                                     : "the text, the record arrays and up to 37 bytes a record for the links, the owners and their grouping do not fit in GPU memory") + sizes);   // the streaming run needs a few blocks of HBM only
    } catch (const DeviceError& e) {
        if (modes) return give_up(e.what());
        announce_handover("the GPU-resident ordered run", e);     // nothing has been written yet
        return false;
    } catch (const std::exception& e) {
        if (modes) if (const DiagnosedError* d = dynamic_cast<const DiagnosedError*>(&e)) std::cerr << d->diag;   // what the host reader found, in full
        return give_up(e.what());                                 // an input the host reader will report on in the reference's words
    }
    // from here on the run is this one's: outputs are created, filled and closed
    OutputFile sink0(out[0]);
    std::unique_ptr<OutputFile> sink1;
    if (S == 2) sink1 = std::make_unique<OutputFile>(out[1]);
    OutputFile* sinks[2] = {&sink0, sink1.get()};
    if (write_clusters_)
        for (int s = 0; s < S; ++s) { write_cluster_lines(clusters[s], out[s] + ".clusters"); std::string().swap(clusters[s]); }
    if (write_levels_) write_cluster_lines(duplevels_text(levels), out[0] + ".duplevels");
    {
        StageClock::Scope t("ordered/resident: survivors out of HBM");
        FileOnDevice* files[2] = {&dev[0], &dev[1]};
        const uint32_t* by_order[2] = {order.p, order.p};
        const uint32_t* idx[2] = {nullptr, nullptr};
        // (the count of pairs that are not written only sizes the windows)
        if (sort_by_size_) write_survivors(eng->e, stream, S, files, by_order, all_kept.p, n_written, 0, sinks, format_, memlimit_, true, &buffers);
        else write_survivors(eng->e, stream, S, files, idx, keep.p, n, dups + dropped_clusters, sinks, format_, memlimit_, true, &buffers);
    }
    if (tuning_.leave_memory_to_exit) g_leave_memory_to_exit = true;
    StageClock::report();
    summary_.total = n; summary_.duplicates = dups; summary_.unmatched = 0;
    if (verbose_) print_summary(S, summary_.total, summary_.duplicates);
    print_not_written(dropped_clusters, dropped_records);
    return true;
}

void HashDupRemover::run_unordered_resident(const std::string* in, const std::string* out)
{
    HIP_OK(hipSetDevice(tuning_.device));
    StreamGuard stream_guard;
    const hipStream_t stream = stream_guard;
    // the engine — key store and table sized from the files' sizes — is made on a helper thread under the reads of the
    // inputs: its first use comes after them (guess_capacity)
    JoinedPairs jp;                                           // (before `eng`: the helper thread makes room in it, and eng's destructor joins that thread first)
    struct LazyEngine {
        std::unique_ptr<EngineHandle> holder; std::thread maker; std::exception_ptr error;
        ~LazyEngine() { if (maker.joinable()) maker.join(); }
        fqd_engine* get() { if (maker.joinable()) maker.join(); if (error) std::rethrow_exception(error); return holder->e; }
    } eng;
    {
        uint64_t cap_reads = 0, cap_bases = 0;
        guess_capacity(2, in, cap_reads, cap_bases);
        eng.maker = std::thread([this, &eng, &jp, stream, cap_reads, cap_bases] {
            try {
                HIP_OK(hipSetDevice(tuning_.device));
                StageClock::Scope t("  on the GPU: engine, key store, table, join arrays (under the read)");
                eng.holder = std::make_unique<EngineHandle>(2, tuning_.device, stream, cap_reads, cap_bases);
                if (cap_reads) jp.prepare(cap_reads);
            }
            catch (...) { eng.error = std::current_exception(); }
        });
    }
    const size_t block_bytes = block_bytes_for(tuning_, memlimit_), fetch_bytes = fetch_bytes_for(block_bytes, memlimit_);

    FileOnDevice dev[2];

    // ---- the one pass: every block to the tail of the file's text in HBM -------------------------------
    {
        StageClock::Scope t("unordered/resident: read, scan, text to HBM");
        // both files at the same time, each on its own thread and copy stream; what goes wrong is still
        // reported in the reference's order: everything about file 1 before anything about file 2 (hpp:161-173)
        std::exception_ptr err[2];
        ParseFailure parse_failure[2];
        auto load = [&](int s) {
            try {
                HIP_OK(hipSetDevice(tuning_.device));
                StreamGuard up;
                uint64_t known = 0;
                if (is_regular_file(in[s], known) && !has_gz_extension(in[s])) dev[s].text.room_for(known + 64, up);   // no regrowth for plain files
                parse_failure[s] = append_file(in[s], format_, true, tuning_.device, block_bytes, dev[s], up);
            } catch (...) { err[s] = std::current_exception(); }
        };
        Fetched got[2];
        auto fetch_or_load = [&](int s) {
            if (inflate_on_device()) {
                try { fetch_file(in[s], fetch_bytes, tuning_.device, dev[s], got[s]); }
                catch (const DeviceOutOfMemory&) { err[s] = std::current_exception(); return; }   // rethrown below: the two-pass run takes over
                catch (const std::exception&) {}                                                  // the host way will say what is wrong
            }
            if (got[s].way == Fetched::None) { got[s].packed = CompressedOnDevice(); dev[s].forget(); load(s); }
        };
        std::thread second(fetch_or_load, 1);
        fetch_or_load(0);
        second.join();
        for (int s = 0; s < 2; ++s) {
            if (got[s].way == Fetched::None) continue;
            StageClock::Scope t2("unordered/resident: inflate + record scan on the GPU");
            if (!cut_records(eng.get(), stream, format_, got[s], dev[s])) {             // read it again the host way: that one reports
                dev[s].forget();
                got[s].packed = CompressedOnDevice();
                load(s);
            }
        }
        for (int s = 0; s < 2; ++s) {
            if (err[s]) std::rethrow_exception(err[s]);
            throw_if_set(parse_failure[s]);
        }
        for (int s = 0; s < 2; ++s) {
            FileOnDevice& f = dev[s];
            f.tag_off.reserve(f.n); f.tag_len.reserve(f.n);
            engine_ok(eng.get(), fqd_extract_tags(eng.get(), reinterpret_cast<const uint8_t*>(f.text.p), f.start.p, f.id_len.p, f.n, f.tag_off.p, f.tag_len.p));
        }
    }

    DeviceSide side[2];
    for (int s = 0; s < 2; ++s) {
        side[s].tag_bytes = side[s].seq_bytes = reinterpret_cast<const uint8_t*>(dev[s].text.p);
        side[s].tag_off = dev[s].tag_off.p; side[s].tag_len = dev[s].tag_len.p;
        side[s].seq_off = dev[s].seq_off.p; side[s].seq_len = dev[s].seq_len.p; side[s].n = dev[s].n;
    }
    // The join, the dedup and every buffer the writer needs come BEFORE the outputs exist: HBM that does not suffice for
    // them (DeviceOutOfMemory) still hands the job to the two-pass run.  On disk nothing differs from the reference's
    // order — outputs opened after the sort phase, then the merge (hpp:265-266) — a bad base found by the dedup cuts the
    // output at the same pair either way.
    fqd_engine* engine_now = eng.get();                        // (joins the helper thread: jp is ours from here on)
    join_and_dedup(engine_now, stream, side, tuning_.reference_tail_rule, jp);
    const uint64_t n_proc = jp.n_proc, upto = std::min<uint64_t>(n_proc, jp.written_below);
    uint64_t dups = 0;
    {
        std::vector<uint8_t> keep(upto);
        if (upto) HIP_OK(hipMemcpyAsync(keep.data(), jp.keep.p, upto, hipMemcpyDeviceToHost, stream));
        HIP_OK(hipStreamSynchronize(stream));
        for (uint64_t k = 0; k < upto; ++k) dups += keep[k] == 0;
    }
    FileOnDevice* files[2] = {&dev[0], &dev[1]};
    const uint32_t* idx[2] = {jp.pair[0].p, jp.pair[1].p};
    SurvivorBuffers buffers;
    {
        const bool gz_out[2] = {has_gz_extension(out[0]), has_gz_extension(out[1])};
        plan_survivors(eng.get(), 2, files, idx, jp.keep.p, upto, gz_out, memlimit_, buffers);
    }

    OutputFile sink0(out[0]), sink1(out[1]);
    OutputFile* sinks[2] = {&sink0, &sink1};

    // ---- outputs: the device assembles windows of survivors in output order, the host writes them -----
    {
        StageClock::Scope t("unordered/resident: survivors out of HBM");
        write_survivors(eng.get(), stream, 2, files, idx, jp.keep.p, upto, dups, sinks, format_, memlimit_, true, &buffers);
    }
    if (tuning_.leave_memory_to_exit) g_leave_memory_to_exit = true;
    StageClock::report();
    if (jp.bad) throw_unknown_base(jp.bad_byte);
    summary_.total = n_proc; summary_.duplicates = dups; summary_.unmatched = jp.unmatched;
    if (verbose_) print_unordered_summary(summary_);
}

} // namespace fqdhost
