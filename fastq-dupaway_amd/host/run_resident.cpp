// run_resident.cpp — the two runs whose text is resident in HBM, ordered (run_ordered_resident) and `--unordered`
// (run_unordered_resident); how the files get there is resident_input.cpp's, what the FQD_FAST_* switches are fast_modes.hpp's.
#include "run_common.hpp"
#include <future>

namespace fqdhost {
using namespace detail;

namespace {

// The engine — its key store and table sized from the files' sizes (guess_capacity) — made on a helper thread under the
// reads of the inputs: its first use comes after them.  also_make(reads) runs on that thread behind it.  get() waits for the
// thread and rethrows what it threw, and so does the destructor of the last copy (the waiting, not the throwing).
using EngineUnderTheRead = std::shared_future<std::shared_ptr<EngineHandle>>;
template <class AlsoMake>
EngineUnderTheRead engine_under_the_read(int S, const std::string* in, int device, hipStream_t stream, const char* stage, AlsoMake also_make)
{
    uint64_t cap_reads = 0, cap_bases = 0;
    guess_capacity(S, in, cap_reads, cap_bases);
    return std::async(std::launch::async, [=] {
        HIP_OK(hipSetDevice(device));
        StageClock::Scope t(stage);
        auto made = std::make_shared<EngineHandle>(S, device, stream, cap_reads, cap_bases);
        also_make(cap_reads);
        return made;
    }).share();
}

// ---- the ordered run, stage by stage --------------------------------------------------------------------------------

// With a switch set (FastModes::any) there is no hand-over: whatever would have sent the input to the streaming run ends
// the run with a message that names the switches and the reason, still before any output exists.
bool give_up(const FastModes& fast, const std::string& why)
{
    if (fast.any()) throw FastModeRefusal(fast.names() + ": the GPU-resident run cannot take this input (" + why + "), and the streaming run cannot serve these modes");
    return false;
}

// Stage 1, decided before any GPU call: whether the run is taken.  Without a switch, only when a codec is involved — a
// BGZF input, or a `.gz` output the GPU can deflate (plain files in and out are better off in the streaming run, where
// reading, the GPU and writing overlap).  With a switch, for plain files as well; nothing: all of them are empty.
bool resident_run_taken(const FastModes& fast, int S, const std::string* in, const std::string* out, bool& nothing)
{
    if (const char* v = std::getenv("FQD_ORDERED_RESIDENT")) if (std::atoi(v) == 0) return give_up(fast, "FQD_ORDERED_RESIDENT=0 turns that run off");
    if (!inflate_on_device()) {
        bool gz = !fast.any();                                    // with a switch set only a `.gz` input needs the device inflate
        for (int s = 0; s < S; ++s) gz |= has_gz_extension(in[s]);
        if (gz) return give_up(fast, "FQD_GUNZIP_DEVICE=0 keeps `.gz` inputs off the GPU");
    }
    bool any_gz_in = false, any_gz_out = false, all_empty = true;
    for (int s = 0; s < S; ++s) {
        uint64_t size = 0;
        if (!is_regular_file(in[s], size)) return give_up(fast, in[s] + " is not a regular file: a pipe cannot be held in GPU memory");
        all_empty &= size == 0;
        any_gz_in |= has_gz_extension(in[s]);
        any_gz_out |= has_gz_extension(out[s]);
    }
    nothing = fast.any() && all_empty;
    return fast.any() || any_gz_in || (any_gz_out && deflate_on_device());
}

// The buffers of a few stages, each released by the scope that ends behind its last reader.
// FQD_FAST_STRAND=both and FQD_FAST_UMI: what the engine is given in place of the reads as they lie in the files, until the
// last submit is through (with FQD_FAST_UMI_MISMATCH the second pass, and the merge, which reads umi_off).
struct KeyedReads {
    Device<uint8_t> canon, turned; Device<uint64_t> canon_off[2]; Device<uint32_t> canon_len[2];   // FQD_FAST_STRAND=both
    Device<uint8_t> umi_text; Device<uint64_t> umi_off64; Device<uint32_t> umi_len, umi_off;        // FQD_FAST_UMI
    fqd_umi_info umi_info{};
    fqd_reads reads[2] = {}, umi_mate{};                         // what is submitted: the given or the canonical reads; mate 1 as `UMI bases ‖ sequence`
};
// Every duplicate's link to an earlier record of its key and the first record of the key, until the records are grouped.
// FQD_FAST_UMI_HAMMING: where every record's UMI field lies and the run's shape, taken over from KeyedReads when that leaves, and
// with FQD_FAST_UMI_MISMATCH the merged owners, which are the molecules' links while `owner` stays the exact owners.
// FQD_FAST_CENTROID=abundant: `exact`, the owners by exact key, which the first stage that replaces them hands over instead of
// letting them leave (4 bytes a record more); they go on to Clusters behind the last grouping.
struct Links { Device<uint32_t> link, owner; Device<uint32_t> umi_off, umi_link, exact; fqd_umi_info umi_info{}; };
// The records grouped by owner: an order of the n records and a flag at the first place of every cluster; with
// FQD_FAST_SIZEIN what every record stands for, while sizes are made.  Until the outputs are planned.
// With FQD_FAST_CENTROID=abundant or =longest the exact owners, and with =longest every record's span (fqd_prefix_merge's
// span_out), until the centroids are picked.
struct Clusters { Device<uint32_t> perm; Device<uint8_t> head; Device<uint32_t> weight, exact, span; uint64_t count = 0; };
// FQD_FAST_OPTICAL: where on the flow cell every record was read (fqd_read_places over file 1's ID lines), until the clusters
// are split.
struct Places {
    Device<uint32_t> tile, x, y, surface; uint64_t other_surface = 0;
    void release() { tile.release(); x.release(); y.release(); surface.release(); }
};

// What lives from stage to stage, in the order it comes to be.  A stage that returns false has found the input one for the
// streaming run (give_up) before any output exists.
struct OrderedResidentRun {
    const FastModes& fast; const int S; const std::string* const in; const std::string* const out;
    const Format format; const long long memlimit; const int device;
    StreamGuard stream;
    FileOnDevice dev[2]; FileOnDevice* files[2] = {&dev[0], &dev[1]};
    uint64_t n = 0, dups = 0;
    Device<uint8_t> keep;
    uint64_t merged_clusters = 0;                                // FQD_FAST_UMI_MISMATCH: the clusters the merge leaves
    uint64_t near_taken = 0;                                     // FQD_FAST_HAMMING: the exact clusters that went into another
    uint64_t umi_near_taken = 0;                                 // FQD_FAST_UMI_HAMMING: the clusters in front of the stage that went into another
    uint64_t prefix_taken = 0;                                   // FQD_FAST_PREFIX: the exact clusters that went into another
    Places places; uint64_t optical_more = 0;                    // FQD_FAST_OPTICAL: the places; the clusters the split adds
    uint64_t centroid_moved = 0;                                 // FQD_FAST_CENTROID=abundant / =longest: the clusters written by another sequence than their first member's
    uint64_t consensus_bases = 0, consensus_reads = 0;           // FQD_FAST_CONSENSUS: the bases replaced, and the records (pairs) that hold them
    std::string cluster_text[2];                                 // FQD_FAST_CLUSTERS
    Device<uint32_t> cluster_size; fqd_size_levels levels{};     // FQD_FAST_SIZEOUT / _LEVELS / _SORT / _MINSIZE / _MAXSIZE
    uint64_t dropped_clusters = 0, dropped_records = 0;          // FQD_FAST_MINSIZE / _MAXSIZE
    Device<uint32_t> order; Device<uint8_t> all_kept;            // FQD_FAST_SORT=size: the written order and a set flag for each of its entries
    // what is written: pair k < upto is record idx[s][k] of file s (nullptr: record k), iff flags[k]; not_written only sizes
    // the writer's windows.  Made once, for plan_survivors and write_survivors alike
    const uint32_t* idx[2] = {nullptr, nullptr}; const uint8_t* flags = nullptr; uint64_t upto = 0, not_written = 0;
    EngineUnderTheRead engine; fqd_engine* e = nullptr;
    SurvivorBuffers buffers;

    OrderedResidentRun(const FastModes& fast_, int S_, const std::string* in_, const std::string* out_, Format format_, long long memlimit_, int device_)
        : fast(fast_), S(S_), in(in_), out(out_), format(format_), memlimit(memlimit_), device(device_) {}

    // Stage 2: the files go to HBM as they lie on disk, on a thread each, while the engine is made; they are inflated (if
    // compressed) and cut into records there.  Only regular files of whole records, as many in file 2 as in file 1, go on.
    bool fetch_and_scan(size_t fetch_bytes, Fetched (&got)[2])
    {
        bool no_room[2] = {false, false};
        std::exception_ptr fetch_error[2];
        engine = engine_under_the_read(S, in, device, stream, "  on the GPU: engine, key store, table (under the read)", [](uint64_t) {});
        {
            StageClock::Scope t("ordered/resident: files to HBM");
            run_parts(unsigned(S), [&](unsigned s) {
                try { fetch_file(in[s], fetch_bytes, device, dev[s], got[s]); }
                catch (const DeviceOutOfMemory&) { no_room[s] = true; }
                catch (const DeviceError&) { fetch_error[s] = std::current_exception(); }
                catch (const std::exception&) {}                           // the host reader will say what is wrong with the file
            });
        }
        engine.wait();
        for (int s = 0; s < S; ++s) if (fetch_error[s]) std::rethrow_exception(fetch_error[s]);
        for (int s = 0; s < S; ++s)
            if (got[s].way == Fetched::None) return give_up(fast, no_room[s] ? in[s] + " does not fit in GPU memory" : in[s] + " could not be taken to GPU memory as it lies on disk (empty, damaged, or changed while it was read)");
        e = engine.get()->e;
        {
            StageClock::Scope t("ordered/resident: inflate + record scan on the GPU");
            for (int s = 0; s < S; ++s)
                if (!cut_records(e, stream, format, got[s], dev[s])) return give_up(fast, in[s] + " does not hold whole, well-formed records");
        }
        if (S == 2 && dev[0].n != dev[1].n) return give_up(fast, "the two files hold different numbers of records");
        n = dev[0].n;
        if (fast.linked() && n >= 0x80000000ull)
            throw FastModeRefusal(fast.names() + ": at most 2^31-1 records (pairs) per run, the input holds " + std::to_string(n));
        if ((fast.both_strands || fast.umi) && n > 0xFFFFFFFEull)
            throw FastModeRefusal(fast.names() + ": at most 2^32-2 records (pairs) per run, the input holds " + std::to_string(n));
        return true;
    }

    // The sequences of file s where the record scan found them in the text.
    fqd_reads reads_as_they_lie(int s) const { return fqd_reads{reinterpret_cast<const uint8_t*>(dev[s].text.p), dev[s].seq_off.p, dev[s].seq_len.p, 0, 0}; }

    // Stage 3, between the record scan and the submit loop.  FQD_FAST_STRAND=both: one fqd_canonical_reads over all n records.
    // FQD_FAST_UMI behind it: fqd_umi_find over file 1's ID lines, then fqd_umi_reads, which packs `UMI bases ‖ sequence` of
    // (the canonical) mate 1 for the submit loop's segment 0.  FQD_FAST_SIZEIN: fqd_size_annotations reads every record's weight
    // off file 1's ID lines and holds file 2 against them.  FQD_FAST_OPTICAL: fqd_read_places reads every record's place off
    // file 1's ID lines.  A record that any of them refuses ends the run.
    void rewrite_keys(KeyedReads& k, Clusters& clusters)
    {
        // no more than a file's sequence bytes — a FASTQ record is its sequence twice (bases, qualities) and at least six
        // more bytes, a FASTA record its sequence and at least three
        auto seq_bound = [&](int s) -> uint64_t {
            return format == Format::Fasta ? dev[s].text.used - std::min<uint64_t>(dev[s].text.used, 3 * n)
                                           : (dev[s].text.used - std::min<uint64_t>(dev[s].text.used, 6 * n)) / 2 + 1;
        };
        for (int s = 0; s < S; ++s) k.reads[s] = reads_as_they_lie(s);
        if (fast.both_strands) {
            // the canonical sequences and their descriptors
            uint64_t bound = 0;
            for (int s = 0; s < S; ++s) bound += seq_bound(s);
            k.canon.reserve(bound + 64); k.turned.reserve(n);
            for (int s = 0; s < S; ++s) { k.canon_off[s].reserve(n); k.canon_len[s].reserve(n); }
            StageClock::Scope t("fast: both strands, canonical reads on the GPU");
            uint64_t n_turned = 0;
            engine_ok<DeviceError>(e, fqd_canonical_reads(e, k.reads, n, k.canon.p, bound, k.canon_off[0].p, k.canon_len[0].p, S == 2 ? k.canon_off[1].p : nullptr,
                                                          S == 2 ? k.canon_len[1].p : nullptr, k.turned.p, StageClock::on() ? &n_turned : nullptr));
            for (int s = 0; s < S; ++s) k.reads[s] = fqd_reads{k.canon.p, k.canon_off[s].p, k.canon_len[s].p, 0, 0};
            if (StageClock::on()) std::cerr << "fast: both strands, " << n_turned << " of " << n << " records turned\n";
        }
        if (fast.umi) {
            StageClock::Scope t("fast: UMI, find and pack on the GPU");
            const uint8_t* text0 = reinterpret_cast<const uint8_t*>(dev[0].text.p);
            k.umi_off.reserve(n);
            fqd_umi_info& info = k.umi_info;
            engine_ok<DeviceError>(e, fqd_umi_find(e, text0, dev[0].start.p, dev[0].id_len.p, n, fast.umi, k.umi_off.p, &info));
            if (info.bad_record != FQD_UMI_NO_RECORD)
                throw FastModeRefusal(fast.umi_name() + ": record " + std::to_string(info.bad_record) + " (counted from 0) of " + in[0] + ": " + umi_reason(info.bad_reason, fast.umi));
            // mate 1's sequence bytes (with both strands the canonical mate 1 of a pair may be either file's read), the UMI
            // bases of every record, and the descriptors
            const uint64_t bound = seq_bound(0) + (fast.both_strands && S == 2 ? seq_bound(1) : 0) + uint64_t(info.n_bases) * n;
            k.umi_text.reserve(bound + 64); k.umi_off64.reserve(n); k.umi_len.reserve(n);
            engine_ok<DeviceError>(e, fqd_umi_reads(e, text0, dev[0].start.p, k.umi_off.p, &info, &k.reads[0], n, k.umi_text.p, bound, k.umi_off64.p, k.umi_len.p));
            k.umi_mate = fqd_reads{k.umi_text.p, k.umi_off64.p, k.umi_len.p, 0, 0};
            if (StageClock::on()) std::cerr << "fast: UMI, " << info.n_bases << " bases behind the last '" << char(fast.umi) << "' of the first word\n";
        }
        if (fast.size_in) {
            // the weights, before anything else is spent on an input with a malformed annotation
            StageClock::Scope t("fast: size annotations on the GPU");
            clusters.weight.reserve(n);
            fqd_sizein_info info{};
            for (int s = 0; s < S; ++s) {
                fqd_sizein_info found{};
                engine_ok<DeviceError>(e, fqd_size_annotations(e, reinterpret_cast<const uint8_t*>(dev[s].text.p), dev[s].start.p, dev[s].id_len.p, n,
                                                               s ? clusters.weight.p : nullptr, s ? nullptr : clusters.weight.p, nullptr, nullptr, &found));
                if (found.bad_record != FQD_UMI_NO_RECORD)
                    throw FastModeRefusal("FQD_FAST_SIZEIN=1: record " + std::to_string(found.bad_record) + " (counted from 0) of " + in[s] + ": " + sizein_reason(found.bad_reason));
                if (s == 0) info = found;
            }
            if (StageClock::on()) std::cerr << "fast: size annotations, " << info.annotated << " of " << n << " records annotated, total weight " << info.total_weight << "\n";
        }
        if (fast.optical) {
            // the places, before anything else is spent on an input whose names hold none
            StageClock::Scope t("fast: optical duplicates, places on the GPU");
            places.tile.reserve(n); places.x.reserve(n); places.y.reserve(n); places.surface.reserve(n);
            fqd_places_info found{};
            engine_ok<DeviceError>(e, fqd_read_places(e, reinterpret_cast<const uint8_t*>(dev[0].text.p), dev[0].start.p, dev[0].id_len.p, n, places.tile.p, places.x.p,
                                                      places.y.p, places.surface.p, &found));
            if (found.bad_record != FQD_UMI_NO_RECORD)
                throw FastModeRefusal(fast.optical_name() + ": record " + std::to_string(found.bad_record) + " (counted from 0) of " + in[0] + ": " + optical_reason(found.bad_reason));
            places.other_surface = found.other_surface;
        }
    }

    // Stage 4: all n records through the engine where they lie, batch by batch; with_umi: mate 1 as `UMI bases ‖ sequence`.
    // The `linked` switches link every duplicate to an earlier record of its key (fqd_submit_linked).
    int submit_all(const KeyedReads& k, Links& links, bool with_umi)
    {
        const size_t kBatch = 16u << 20;
        int rc = FQD_OK;
        for (size_t a = 0; a < n && rc == FQD_OK; a += kBatch) {
            fqd_reads seg[2] = {with_umi ? k.umi_mate : k.reads[0], k.reads[1]};
            for (int s = 0; s < S; ++s) { seg[s].offsets += a; seg[s].lengths += a; }
            if (fast.linked()) rc = fqd_submit_linked(e, seg, std::min<size_t>(kBatch, n - a), FQD_MEM_DEVICE, keep.p + a, links.link.p + a, a + kBatch < n ? 0 : 1);
            else rc = (a + kBatch < n ? fqd_submit : fqd_submit_final)(e, seg, std::min<size_t>(kBatch, n - a), FQD_MEM_DEVICE, keep.p + a);
        }
        if (rc == FQD_OK) rc = fqd_engine_sync(e);
        return rc;
    }

    bool first_pass(const KeyedReads& k, Links& links)
    {
        const int rc = submit_all(k, links, fast.umi != 0);
        if (rc == FQD_ERR_BAD_BASE)                                  // the streaming run cuts the output where the reference does
            return give_up(fast, std::string(fqd_last_error(e)) + (fast.umi ? "; a position in mate 1 counts the " + std::to_string(k.umi_info.n_bases) + " UMI bases in front of the sequence" : std::string()));
        if (rc != FQD_OK) throw DeviceError(std::string("GPU engine: ") + fqd_last_error(e));
        return true;
    }

    // Stage 5, FQD_FAST_UMI_MISMATCH=1|2 (FQD_FAST_UMI is set): the engine is used TWICE.  The first pass, keyed `UMI bases ‖
    // sequence`, gives the exact owners and, through fqd_group_owners and the sizes, every exact cluster's count; after
    // fqd_engine_reset the same batches go in again keyed by the sequences alone, into the same flags and links — those of the
    // first pass are used up by fqd_owners — which gives every record's sequence group.  fqd_umi_merge makes the merged owners
    // of the three, fqd_owners_to_keep the flags; the merged owners are THE owners from here on.  With FQD_FAST_UMI_HAMMING the
    // exact owners stay THE owners — the nodes of merge_near_umi — and the merged ones are kept beside them as its links.
    void merge_umi_neighbours(const KeyedReads& k, Links& links, Clusters& clusters)
    {
        Device<uint32_t> owner_seq, exact_size, merged_owner;
        owner_seq.reserve(n); exact_size.reserve(n); merged_owner.reserve(n);
        uint64_t exact_clusters = 0;
        {
            StageClock::Scope t("fast: UMI mismatches, exact owners and counts on the GPU");
            engine_ok<DeviceError>(e, fqd_owners(e, keep.p, links.link.p, n, links.owner.p));
            engine_ok<DeviceError>(e, fqd_group_owners(e, links.owner.p, n, clusters.perm.p, clusters.head.p, &exact_clusters));
            cluster_sizes(clusters, exact_size.p, nullptr);
        }
        {
            StageClock::Scope t("fast: UMI mismatches, second pass by sequence on the GPU");
            engine_ok<DeviceError>(e, fqd_engine_reset(e));
            if (submit_all(k, links, false) != FQD_OK) throw DeviceError(std::string("GPU engine: ") + fqd_last_error(e));
            engine_ok<DeviceError>(e, fqd_owners(e, keep.p, links.link.p, n, owner_seq.p));
        }
        StageClock::Scope t("fast: UMI mismatches, networks on the GPU");
        fqd_umi_merge_info merged{};
        engine_ok<DeviceError>(e, fqd_umi_merge(e, reinterpret_cast<const uint8_t*>(dev[0].text.p), dev[0].start.p, k.umi_off.p, &k.umi_info, links.owner.p,
                                                owner_seq.p, exact_size.p, n, uint32_t(fast.umi_mismatch), merged_owner.p, &merged));
        if (merged.over_limit_first != FQD_UMI_NO_RECORD)
            throw FastModeRefusal(fast.mismatch_name() + ": the sequence of record " + std::to_string(merged.over_limit_first) + " (counted from 0) of " + in[0] + " stands under " +
                                  std::to_string(merged.over_limit_nodes) + " different UMIs, a network of at most " + std::to_string(merged.max_group) +
                                  " is merged (amplicon-style data: deduplicate it by exact UMI, without the switch)");
        if (merged.nodes != exact_clusters) throw DeviceError("GPU engine: internal error (the merge and the grouping count different exact clusters)");
        engine_ok<DeviceError>(e, fqd_owners_to_keep(e, merged_owner.p, n, keep.p));
        if (StageClock::on())
            std::cerr << "fast: UMI mismatches <= " << fast.umi_mismatch << ", " << merged.merged << " of " << merged.nodes << " exact clusters merged into others, largest network "
                      << merged.largest << ", " << merged.sweeps << " sweeps\n";
        merged_clusters = merged.nodes - merged.merged;
        if (fast.umi_hamming) links.umi_link.swap(merged_owner);     // (4 bytes a record more: the exact owners stay)
        else { links.owner.swap(merged_owner); keep_exact(links, merged_owner); }   // (the exact owners leave with this stage, or stay for the centroids)
    }

    // FQD_FAST_CENTROID=abundant / =longest: `replaced` holds the owners a stage has just replaced.  Those of the FIRST stage that replaces any
    // are the owners by exact key, and stay; a later stage's (the optical split behind a merge) are merged ones, and leave.
    void keep_exact(Links& links, Device<uint32_t>& replaced)
    {
        if (fast.picks_centroid() && !links.exact.p) links.exact.swap(replaced);
    }

    // The tail of merge_near, merge_near_umi, merge_prefixes and split_optical: new_owner become THE owners (the replaced ones leave with the
    // caller's buffer, or stay for the centroids), fqd_owners_to_keep makes the flags of them and fqd_group_owners groups the
    // records once more, into the clusters the stage counted.  what: "merge" / "split", for the message.
    void regroup_under(Links& links, Clusters& clusters, Device<uint32_t>& new_owner, uint64_t expected, const char* what)
    {
        links.owner.swap(new_owner);
        keep_exact(links, new_owner);
        engine_ok<DeviceError>(e, fqd_owners_to_keep(e, links.owner.p, n, keep.p));
        engine_ok<DeviceError>(e, fqd_group_owners(e, links.owner.p, n, clusters.perm.p, clusters.head.p, &clusters.count));
        if (clusters.count != expected)
            throw DeviceError(std::string("GPU engine: internal error (the ") + what + " and the second grouping count different clusters)");
    }

    // Stage 6: the duplicates are counted and, for the `linked` switches, the links resolved to the first record of every key
    // (fqd_owners; done already where the merge made the owners) and the records grouped by it (fqd_group_owners) ...
    void count_and_group(Links& links, Clusters& clusters)
    {
        fqd_stats st{};
        fqd_get_stats(e, &st);
        dups = fast.umi_mismatch ? n - merged_clusters : st.duplicates;
        if (!fast.linked()) return;
        {
            StageClock::Scope t("fast: owners and clusters on the GPU");
            if (!fast.umi_mismatch) engine_ok<DeviceError>(e, fqd_owners(e, keep.p, links.link.p, n, links.owner.p));
            engine_ok<DeviceError>(e, fqd_group_owners(e, links.owner.p, n, clusters.perm.p, clusters.head.p, &clusters.count));
        }
        if (fast.hamming) { merge_near(links, clusters); dups = n - clusters.count; }
        if (fast.umi_hamming) { merge_near_umi(links, clusters); dups = n - clusters.count; }
        if (fast.prefix) { merge_prefixes(links, clusters); dups = n - clusters.count; }
        if (fast.optical) { split_optical(links, clusters); dups = n - clusters.count; }
        if (clusters.count + dups != n) throw DeviceError("GPU engine: internal error (the clusters and the duplicates do not add up to the records)");
        if (fast.picks_centroid()) clusters.exact.swap(links.exact); // (check() has seen to it that a merge ran)
    }

    // FQD_FAST_HAMMING, behind the grouping: fqd_near_merge makes of the exact clusters — the reads as they lie in the files, the
    // owners by key — the merged ones, each owned by its first record; regroup_under makes the merged owners THE owners.
    void merge_near(Links& links, Clusters& clusters)
    {
        Device<uint32_t> merged_owner;
        merged_owner.reserve(n);
        const fqd_reads reads[2] = {reads_as_they_lie(0), S == 2 ? reads_as_they_lie(1) : fqd_reads{}};
        fqd_near_info merged{};
        {
            StageClock::Scope t("fast: substitutions, exact clusters merged on the GPU");
            engine_ok<DeviceError>(e, fqd_near_merge(e, reads, links.owner.p, n, fast.hamming, 0, merged_owner.p, &merged));
            if (merged.over_limit_first != FQD_UMI_NO_RECORD)
                throw FastModeRefusal(fast.hamming_name() + ": " + std::to_string(merged.over_limit_nodes) + " different sequences, the one of record " +
                                      std::to_string(merged.over_limit_first) + " (counted from 0) of " + in[0] + " the first among them, share one of the " +
                                      std::to_string(fast.hamming + 1) + " segments their first mate is cut into; a group of at most " + std::to_string(merged.max_group) +
                                      " is compared (adapter dimers, amplicons: trim the reads or dereplicate them exactly first)");
            if (merged.nodes != clusters.count) throw DeviceError("GPU engine: internal error (the merge and the grouping count different exact clusters)");
            regroup_under(links, clusters, merged_owner, merged.merged, "merge");   // (the owners by key leave with this stage, or stay for the centroids)
        }
        near_taken = merged.nodes - merged.merged;
        if (StageClock::on())
            std::cerr << "fast: substitutions <= " << fast.hamming << ", " << near_taken << " of " << merged.nodes << " exact clusters merged into others, " << merged.pairs
                      << " pairs compared, " << merged.edges << " near, largest seed group " << merged.largest_group << ", " << merged.sweeps << " sweeps\n";
    }

    // FQD_FAST_UMI_HAMMING, behind the grouping, where merge_near stands (the two never run together): fqd_near_merge_umi makes of
    // the exact clusters of the run keyed `UMI bases ‖ sequence` — the reads as they lie in the files, the exact owners, every
    // record's UMI field and, with FQD_FAST_UMI_MISMATCH, the merged owners as links — the molecules, each owned by its first
    // record; regroup_under makes their owners THE owners.  The clusters in front of the stage are the exact ones, or the merge's.
    void merge_near_umi(Links& links, Clusters& clusters)
    {
        Device<uint32_t> merged_owner;
        merged_owner.reserve(n);
        const fqd_reads reads[2] = {reads_as_they_lie(0), S == 2 ? reads_as_they_lie(1) : fqd_reads{}};
        const uint64_t before = fast.umi_mismatch ? merged_clusters : clusters.count;
        fqd_near_umi_info merged{};
        {
            StageClock::Scope t("fast: UMI substitutions, exact clusters merged on the GPU");
            engine_ok<DeviceError>(e, fqd_near_merge_umi(e, reads, links.owner.p, fast.umi_mismatch ? links.umi_link.p : nullptr, n, fast.umi_hamming, 0,
                                                         reinterpret_cast<const uint8_t*>(dev[0].text.p), dev[0].start.p, links.umi_off.p, &links.umi_info, merged_owner.p,
                                                         &merged));
            if (merged.near.over_limit_first != FQD_UMI_NO_RECORD)
                throw FastModeRefusal(fast.umi_hamming_name() + ": " + std::to_string(merged.near.over_limit_nodes) + " different sequences under one UMI, the one of record " +
                                      std::to_string(merged.near.over_limit_first) + " (counted from 0) of " + in[0] + " the first among them, share one of the " +
                                      std::to_string(fast.umi_hamming + 1) + " segments their first mate is cut into; a group of at most " +
                                      std::to_string(merged.near.max_group) + " is compared (adapter dimers, amplicons: trim the reads, or run without the switch)");
            if (merged.near.nodes != clusters.count) throw DeviceError("GPU engine: internal error (the merge and the grouping count different exact clusters)");
            if (merged.near.nodes - merged.links != before) throw DeviceError("GPU engine: internal error (the links and the merged UMI clusters differ in number)");
            links.umi_link.release(); links.umi_off.release();
            regroup_under(links, clusters, merged_owner, merged.near.merged, "merge");   // (the exact owners leave with this stage, or stay for the centroids)
        }
        umi_near_taken = before - merged.near.merged;
        if (StageClock::on())
            std::cerr << "fast: UMI substitutions <= " << fast.umi_hamming << ", " << umi_near_taken << " of " << before << " clusters merged into others, " << merged.near.pairs
                      << " pairs compared, " << merged.near.edges << " near, " << merged.links << " links, largest seed group " << merged.near.largest_group << ", "
                      << merged.near.sweeps << " sweeps\n";
    }

    // FQD_FAST_PREFIX, behind the grouping, where merge_near stands (check() sees to it that the two never run together):
    // fqd_prefix_merge makes of the exact clusters — the reads as they lie in the files, the owners by key — the trees of the
    // prefix relation, each owned by its first record; regroup_under makes the merged owners THE owners.  With
    // FQD_FAST_CENTROID=longest every record's span comes back with them, for pick_centroids.
    void merge_prefixes(Links& links, Clusters& clusters)
    {
        Device<uint32_t> merged_owner;
        merged_owner.reserve(n);
        if (fast.longest) clusters.span.reserve(n);
        const fqd_reads reads[2] = {reads_as_they_lie(0), S == 2 ? reads_as_they_lie(1) : fqd_reads{}};
        fqd_prefix_info merged{};
        {
            StageClock::Scope t("fast: prefixes, exact clusters merged on the GPU");
            engine_ok<DeviceError>(e, fqd_prefix_merge(e, reads, links.owner.p, n, fast.prefix, 0, merged_owner.p, fast.longest ? clusters.span.p : nullptr, &merged));
            if (merged.over_limit_first != FQD_UMI_NO_RECORD)
                throw FastModeRefusal(fast.prefix_name() + ": " + std::to_string(merged.over_limit_nodes) + " different sequences, the one of record " +
                                      std::to_string(merged.over_limit_first) + " (counted from 0) of " + in[0] + " the first among them, begin with the same " +
                                      std::to_string(fast.prefix) + (S == 1 ? " bases" : " bases in each mate") + "; a group of at most " + std::to_string(merged.max_group) +
                                      " is compared (adapter dimers, amplicons: set a larger FQD_FAST_PREFIX, or trim the reads first)");
            if (merged.nodes != clusters.count) throw DeviceError("GPU engine: internal error (the merge and the grouping count different exact clusters)");
            regroup_under(links, clusters, merged_owner, merged.merged, "merge");   // (the owners by key leave with this stage, or stay for the centroids)
        }
        prefix_taken = merged.nodes - merged.merged;
        if (StageClock::on())
            std::cerr << "fast: prefixes >= " << fast.prefix << ", " << prefix_taken << " of " << merged.nodes << " exact clusters merged into others, " << merged.pairs
                      << " pairs compared, " << merged.related << " related, largest seed group " << merged.largest_group << ", deepest chain " << merged.deepest << ", "
                      << merged.jumps << " jumps\n";
    }

    // FQD_FAST_OPTICAL, behind the grouping (and the merges, where they run): fqd_optical_split makes of every cluster its
    // optical groups, each owned by its first member; regroup_under makes the split owners THE owners.  The places leave with this stage.
    void split_optical(Links& links, Clusters& clusters)
    {
        Device<uint32_t> split_owner;
        split_owner.reserve(n);
        fqd_optical_info split{};
        {
            StageClock::Scope t("fast: optical duplicates, clusters split on the GPU");
            engine_ok<DeviceError>(e, fqd_optical_split(e, clusters.perm.p, clusters.head.p, reinterpret_cast<const uint8_t*>(dev[0].text.p), dev[0].start.p, places.tile.p,
                                                        places.x.p, places.y.p, places.surface.p, n, fast.optical, split_owner.p, &split));
            if (split.over_limit_first != FQD_UMI_NO_RECORD)
                throw FastModeRefusal(fast.optical_name() + ": the cluster of record " + std::to_string(split.over_limit_first) + " (counted from 0) of " + in[0] + " holds " +
                                      std::to_string(split.over_limit_members) + " identical reads, a cluster of at most " + std::to_string(split.max_cluster) +
                                      " is split (untrimmed poly-G and the like: trim the reads first)");
            if (split.clusters_in != clusters.count) throw DeviceError("GPU engine: internal error (the split and the grouping count different clusters)");
            regroup_under(links, clusters, split_owner, split.clusters_out, "split");   // (the owners by key leave with this stage; behind a merge its exact owners are held already)
        }
        optical_more = split.clusters_out - split.clusters_in;
        if (StageClock::on())
            std::cerr << "fast: optical duplicates within " << fast.optical << " pixels, " << split.split << " of " << split.clusters_in << " clusters split, " << optical_more
                      << " more written, largest cluster " << split.largest << ", " << split.sweeps << " sweeps, " << places.other_surface
                      << " records on another surface than record 0\n";
        places.release();
    }

    // fqd_cluster_sizes: the member count of every cluster at the record that is written, 4 bytes a record, and the level
    // table; with FQD_FAST_SIZEIN fqd_cluster_weights stands in its place: a cluster above 2^31-1 ends the run.
    void cluster_sizes(const Clusters& c, uint32_t* size, fqd_size_levels* lv)
    {
        if (!fast.size_in) { engine_ok<DeviceError>(e, fqd_cluster_sizes(e, c.perm.p, c.head.p, n, size, lv)); return; }
        fqd_weights_info over{};
        engine_ok<DeviceError>(e, fqd_cluster_weights(e, c.perm.p, c.head.p, c.weight.p, n, size, lv, &over));
        if (over.over_record != FQD_UMI_NO_RECORD)
            throw FastModeRefusal("FQD_FAST_SIZEIN=1: the cluster of record " + std::to_string(over.over_record) + " (counted from 0) of " + in[0] + " has the weighted size " +
                                  std::to_string(over.over_sum) + ": at most 2147483647");
    }

    // FQD_FAST_CONSENSUS, directly behind the pick: fqd_consensus per file over the text where it lies in HBM — the written member
    // of every cluster of two or more gets the cluster's consensus as its sequence and quality lines, of the same lengths, so
    // that the plan, the writer, the labels and the deflate see a text like any other.  A pair is counted once through `changed`.
    void vote_consensus(const Clusters& c)
    {
        StageClock::Scope t("fast: consensus of the clusters on the GPU");
        Device<uint8_t> changed;
        if (S == 2) { changed.reserve(n); HIP_OK(hipMemsetAsync(changed.p, 0, n, stream)); }
        fqd_consensus_info voted{};
        for (int s = 0; s < S; ++s) {
            fqd_consensus_info one{};
            engine_ok<DeviceError>(e, fqd_consensus(e, c.perm.p, c.head.p, n, reinterpret_cast<uint8_t*>(dev[s].text.p), dev[s].start.p, dev[s].size.p, dev[s].seq_off.p,
                                                    dev[s].seq_len.p, 0, S == 2 ? changed.p : nullptr, &one));
            voted = one;
            consensus_bases += one.bases_changed; consensus_reads += one.reads_changed;
        }
        if (StageClock::on())
            std::cerr << "fast: consensus, " << voted.clusters << " clusters of " << voted.members << " records voted, largest " << voted.largest << ", " << consensus_bases
                      << " bases in " << consensus_reads << (S == 1 ? " reads" : " read pairs") << " replaced\n";
    }

    // FQD_FAST_CENTROID=abundant, in front of everything that reads which member is written: fqd_subcluster_sizes gives every record
    // the weight of its exact key's copies inside its cluster, fqd_seq_pick_best over them puts the first copy of the most
    // abundant at the head's place.  With FQD_FAST_KEEP=best the scores are then masked to that sequence's copies
    // (fqd_subcluster_scores) and picked from in place of the pick over the whole cluster.  The exact owners and the
    // abundances leave with this stage.
    // FQD_FAST_CENTROID=longest (with FQD_FAST_PREFIX): the spans stand in the place of the abundances — a span is constant on
    // an exact sub-cluster and a tree's largest is its root's alone, so the same pick puts the first copy of the root sequence at
    // the head's place — and everything behind the pick is the same.
    void pick_centroids(Clusters& c)
    {
        if (fast.longest) {
            {
                StageClock::Scope t("fast: longest sequence on the GPU");
                engine_ok<DeviceError>(e, fqd_seq_pick_best(e, c.span.p, c.head.p, n, c.perm.p, &centroid_moved));
            }
            c.span.release();
            if (StageClock::on()) std::cerr << "fast: longest sequence, " << centroid_moved << " of " << c.count << " clusters changed\n";
        } else {
            fqd_centroid_info found{};
            {
                StageClock::Scope t("fast: most abundant sequence on the GPU");
                Device<uint32_t> abundance;
                abundance.reserve(n);
                engine_ok<DeviceError>(e, fqd_subcluster_sizes(e, c.perm.p, c.head.p, c.exact.p, fast.size_in ? c.weight.p : nullptr, n, abundance.p, &found));
                engine_ok<DeviceError>(e, fqd_seq_pick_best(e, abundance.p, c.head.p, n, c.perm.p, &centroid_moved));
            }
            if (StageClock::on())
                std::cerr << "fast: most abundant sequence, " << centroid_moved << " of " << c.count << " clusters changed, " << found.mixed << " mixed clusters, "
                          << found.subclusters << " sub-clusters, largest cluster " << found.largest << "\n";
        }
        if (fast.keep_best) {
            StageClock::Scope t("fast: best-quality pick on the GPU");
            fqd_tags recs[2];
            for (int s = 0; s < S; ++s) recs[s] = fqd_tags{reinterpret_cast<const uint8_t*>(dev[s].text.p), dev[s].start.p, dev[s].size.p, n};
            Device<uint32_t> score, masked;
            score.reserve(n); masked.reserve(n);
            uint64_t moved = 0;
            engine_ok<DeviceError>(e, fqd_seq_scores(e, &recs[0], S == 2 ? &recs[1] : nullptr, score.p));
            engine_ok<DeviceError>(e, fqd_subcluster_scores(e, c.perm.p, c.head.p, c.exact.p, score.p, n, masked.p));
            engine_ok<DeviceError>(e, fqd_seq_pick_best(e, masked.p, c.head.p, n, c.perm.p, &moved));
            if (StageClock::on()) std::cerr << "fast: best-quality pick, " << moved << " of " << c.count << " clusters changed\n";
        }
        c.exact.release();
        engine_ok<DeviceError>(e, fqd_heads_to_keep(e, c.perm.p, c.head.p, n, keep.p));
    }

    // ... then, while perm and head exist: FQD_FAST_CENTROID=abundant picks the centroids (pick_centroids, which does
    // FQD_FAST_KEEP=best's part as well); otherwise FQD_FAST_KEEP=best moves the keep flag of every cluster to its best member
    // (pick_best_members, fqd_heads_to_keep); FQD_FAST_CONSENSUS votes (vote_consensus); FQD_FAST_CLUSTERS takes the clusters' ID lines; the sizes are made for whatever
    // reads them (FastModes::sized), and the weights released behind them; fqd_size_filter clears the flags of the clusters
    // outside the bounds — behind the cluster files and the level table, which hold all clusters; fqd_size_order writes the
    // records that stay in order of decreasing cluster size.  The sizes stay for the writer with FQD_FAST_SIZEOUT only.
    void pick_size_filter_order(Clusters& c)
    {
        if (fast.picks_centroid()) pick_centroids(c);
        else if (fast.keep_best) {
            const uint64_t moved = pick_best_members(e, S, files, n, c.head.p, c.perm.p, "fast: best-quality pick on the GPU");
            engine_ok<DeviceError>(e, fqd_heads_to_keep(e, c.perm.p, c.head.p, n, keep.p));
            if (StageClock::on()) std::cerr << "fast: best-quality pick, " << moved << " of " << c.count << " clusters changed\n";
        }
        if (fast.consensus) vote_consensus(c);
        if (fast.clusters) {
            StageClock::Scope t("fast: ID lines of the clusters out of HBM");
            for (int s = 0; s < S; ++s) cluster_text[s] = cluster_lines(e, stream, dev[s], c.perm.p, c.head.p, n);
        }
        if (fast.sized()) {
            StageClock::Scope t("fast: cluster sizes on the GPU");
            cluster_size.reserve(n);
            cluster_sizes(c, cluster_size.p, &levels);
            c.weight.release();
            if (StageClock::on()) std::cerr << "fast: cluster sizes, " << c.count << " clusters, largest " << levels.largest << "\n";
        }
        if (fast.size_filter()) {
            StageClock::Scope t("fast: size filter on the GPU");
            engine_ok<DeviceError>(e, fqd_size_filter(e, cluster_size.p, n, fast.min_size, fast.max_size, keep.p, &dropped_clusters, &dropped_records));
            if (StageClock::on()) std::cerr << "fast: size filter, " << dropped_clusters << " clusters of " << dropped_records << " records not written\n";
        }
        if (fast.sort_by_size) {
            const uint64_t stay = c.count - dropped_clusters;
            order.reserve(std::max<uint64_t>(stay, 1)); all_kept.reserve(std::max<uint64_t>(stay, 1));    // (a filter may leave nothing)
            fqd_size_order_info sorted{};
            {
                StageClock::Scope t("fast: abundance order on the GPU");
                engine_ok<DeviceError>(e, fqd_size_order_ex(e, c.perm.p, c.head.p, cluster_size.p, keep.p, n, order.p, &upto, &sorted));
                if (upto != stay) throw DeviceError("GPU engine: internal error (the written order and the kept clusters differ in number)");
                if (upto) HIP_OK(hipMemsetAsync(all_kept.p, 1, upto, stream));
                HIP_OK(hipStreamSynchronize(stream));
            }
            // (what the call counted: the pairs of tier 1's bucket 0, which alone went through tier 2's passes)
            if (StageClock::on()) std::cerr << "fast: abundance order, " << upto << " clusters written, " << sorted.large << " of them above 255 members sorted apart\n";
            // pair k is record order[k], of both files; every pair is written
            idx[0] = idx[1] = order.p; flags = all_kept.p;
            buffers.record_keep = keep.p; buffers.records = n;
        }
        if (!fast.size_out) cluster_size.release();
    }

    // Stage 7: everything the writer needs is reserved HERE, while the run can still hand over: once an output exists it
    // cannot.  With FQD_FAST_SORT=size pair k is record order[k] of both files and every pair is written — the labels of
    // FQD_FAST_SIZEOUT are still found per record and brought into the order by the writer (survivor_writer.cpp), which has the
    // sizes in written order once the plan is made.  A filter alone needs no index: the cleared flags go through the plan.
    void plan()
    {
        bool gz_out[2] = {false, false};
        for (int s = 0; s < S; ++s) gz_out[s] = has_gz_extension(out[s]);
        if (fast.size_out) { buffers.cluster_size = cluster_size.p; buffers.size_in = fast.size_in; }
        if (!fast.sort_by_size) { flags = keep.p; upto = n; not_written = dups + dropped_clusters; }
        plan_survivors(e, S, files, idx, flags, upto, gz_out, memlimit, buffers);
        if (fast.sort_by_size) cluster_size.release();
    }

    // Stage 8: from here on the run is this one's: outputs are created, filled and closed — the survivors in the written
    // order window by window (deflated on the device for `.gz` outputs), the cluster files and the level table beside them.
    void write()
    {
        std::unique_ptr<OutputFile> sink[2];
        for (int s = 0; s < S; ++s) sink[s] = std::make_unique<OutputFile>(out[s]);
        OutputFile* sinks[2] = {sink[0].get(), sink[1].get()};
        if (fast.clusters)
            for (int s = 0; s < S; ++s) { write_cluster_lines(cluster_text[s], out[s] + ".clusters"); std::string().swap(cluster_text[s]); }
        if (fast.levels) write_cluster_lines(duplevels_text(levels), out[0] + ".duplevels");
        StageClock::Scope t("ordered/resident: survivors out of HBM");
        write_survivors(e, stream, S, files, idx, flags, upto, not_written, sinks, format, memlimit, true, &buffers);
    }
};

} // namespace

// Everything about the seventeen switches that their values and the command line decide, before any GPU call.
void HashDupRemover::read_fast_modes(bool unordered)
{
    fast_ = FastModes::from_env();
    fast_.check(unordered, tuning_.devices.size(), format_);
    if (fast_.any() && tuning_.devices.size() == 1) { tuning_.device = tuning_.devices[0]; tuning_.devices.clear(); }
}

// An ordered run (single-end, or paired files read side by side) with a codec at either end — BGZF inputs, or `.gz`
// outputs of plain regular inputs — or with a FQD_FAST_* switch set: every read (pair) is deduplicated where it lies in
// HBM, and the survivors leave window by window.  false: not taken, returned BEFORE any output is touched, and the
// streaming run (run_ordered), which reproduces the reference's behaviour for every irregular input, does the job.
bool HashDupRemover::run_ordered_resident(int S, const std::string* in, const std::string* out)
{
    bool nothing = false;
    if (!resident_run_taken(fast_, S, in, out, nothing)) return false;                                       // stage 1
    if (nothing) {
        // no record, no cluster, nothing to choose: what the default run makes of empty files, and empty cluster files
        // (the table of zeros is written whatever the default run makes of an empty file, behind its outputs)
        struct LevelsOfNothing { bool on; const std::string& name; ~LevelsOfNothing() { if (on) write_cluster_lines(duplevels_text(fqd_size_levels{}), name + ".duplevels"); } }
            levels_of_nothing{fast_.levels, out[0]};
        run_ordered(S, in, out);                                  // (no cluster, no filter: the second `-v` line is not said either)
        if (fast_.clusters) for (int s = 0; s < S; ++s) write_cluster_lines(std::string(), out[s] + ".clusters");
        return true;
    }
    HIP_OK(hipSetDevice(tuning_.device));
    OrderedResidentRun run(fast_, S, in, out, format_, memlimit_, tuning_.device);
    const uint64_t& n = run.n;
    try {
        // (way None: not fetched, an exception included.  A BGZF file's packed bytes stay until the outputs are planned:
        // gigabytes freed in mid-run are cleared by the driver while the process's next hipMalloc waits)
        Fetched got[2];
        if (!run.fetch_and_scan(fetch_bytes_for(block_bytes_for(tuning_, memlimit_), memlimit_), got)) return false;   // stage 2
        StageClock::Scope t("ordered/resident: dedup on the GPU");
        run.keep.reserve(n);
        {
            Clusters clusters;
            {
                Links links;
                if (fast_.linked()) { links.link.reserve(n); links.owner.reserve(n); clusters.perm.reserve(n); clusters.head.reserve(n); }
                {
                    KeyedReads keyed;
                    run.rewrite_keys(keyed, clusters);                                                       // stage 3
                    if (!run.first_pass(keyed, links)) return false;                                         // stage 4
                    if (fast_.umi_mismatch) run.merge_umi_neighbours(keyed, links, clusters);                // stage 5
                    if (fast_.umi_hamming) { links.umi_off.swap(keyed.umi_off); links.umi_info = keyed.umi_info; }   // (merge_near_umi reads them in stage 6)
                }
                if (std::getenv("FQD_TEST_FAIL_RESIDENT")) throw DeviceError("GPU engine: forced by FQD_TEST_FAIL_RESIDENT");      // tests: the hand-over is announced
                run.count_and_group(links, clusters);                                                        // stage 6 ...
            }
            if (fast_.linked()) run.pick_size_filter_order(clusters);
        }
        run.plan();                                                                                          // stage 7
    } catch (const FastModeRefusal&) {
        throw;                                                    // nothing has been written
    } catch (const DeviceOutOfMemory&) {
        return give_up(fast_, fast_.out_of_memory_note());        // (the streaming run needs a few blocks of HBM only)
    } catch (const DeviceError& e) {
        if (fast_.any()) return give_up(fast_, e.what());
        announce_handover("the GPU-resident ordered run", e);     // nothing has been written yet
        return false;
    } catch (const std::exception& e) {
        if (fast_.any()) if (const DiagnosedError* d = dynamic_cast<const DiagnosedError*>(&e)) std::cerr << d->diag;   // what the host reader found, in full
        return give_up(fast_, e.what());                          // an input the host reader will report on in the reference's words
    }
    run.write();                                                                                             // stage 8
    if (tuning_.leave_memory_to_exit) g_leave_memory_to_exit = true;
    StageClock::report();
    summary_.total = run.n; summary_.duplicates = run.dups; summary_.unmatched = 0;
    if (verbose_) print_summary(S, summary_.total, summary_.duplicates);
    // FQD_FAST_HAMMING: what `-v` says behind its first line, which counts every record that was not written
    if (verbose_ && fast_.hamming)
        std::cout << run.near_taken << (S == 1 ? " distinct sequences" : " distinct sequence pairs") << " were taken for copies of another that differs in at most " << fast_.hamming
                  << (S == 1 ? " bases (" : " bases a mate (") << fast_.hamming_name() << ").\n";
    // FQD_FAST_UMI_HAMMING: what `-v` says behind its first line, which counts every record that was not written
    if (verbose_ && fast_.umi_hamming)
        std::cout << run.umi_near_taken << (S == 1 ? " distinct sequences" : " distinct sequence pairs") << " under one UMI were taken for copies of another that differs in at most "
                  << fast_.umi_hamming << (S == 1 ? " bases (" : " bases a mate (") << fast_.umi_hamming_name() << ").\n";
    // FQD_FAST_PREFIX: what `-v` says behind its first line, which counts every record that was not written
    if (verbose_ && fast_.prefix)
        std::cout << run.prefix_taken << (S == 1 ? " distinct sequences" : " distinct sequence pairs") << " were taken for copies of a longer " << (S == 1 ? "sequence" : "sequence pair")
                  << " that begins with them" << (S == 1 ? "" : ", mate by mate") << ", over at least " << fast_.prefix << (S == 1 ? " bases (" : " bases a mate (") << fast_.prefix_name()
                  << ").\n";
    // FQD_FAST_OPTICAL: what `-v` says behind its first line, which counts the optical duplicates only
    if (verbose_ && fast_.optical)
        std::cout << run.optical_more << (S == 1 ? " reads" : " read pairs") << " that repeat an earlier sequence were written: not optical duplicates (" << fast_.optical_name() << ").\n";
    // FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE: what `-v` says behind these
    if (verbose_ && fast_.size_filter())
        std::cout << run.dropped_clusters << " clusters holding " << run.dropped_records << (S == 1 ? " reads" : " read pairs") << " were not written (FQD_FAST_MINSIZE=" << fast_.min_size
                  << ", FQD_FAST_MAXSIZE=" << (fast_.max_size ? std::to_string(fast_.max_size) : std::string("none")) << ").\n";
    // FQD_FAST_CENTROID=abundant: what `-v` says behind those
    if (verbose_ && fast_.centroid)
        std::cout << run.centroid_moved << " clusters were written by a copy of their most abundant " << (S == 1 ? "sequence" : "sequence pair") << ", not by their first "
                  << (S == 1 ? "read" : "read pair") << " (FQD_FAST_CENTROID=abundant).\n";
    // FQD_FAST_CONSENSUS: what `-v` says behind those
    if (verbose_ && fast_.longest)
        std::cout << run.centroid_moved << " clusters were written by a copy of their longest " << (S == 1 ? "sequence" : "sequence pair") << ", not by their first "
                  << (S == 1 ? "read" : "read pair") << " (FQD_FAST_CENTROID=longest).\n";
    if (verbose_ && fast_.consensus)
        std::cout << run.consensus_bases << " bases in " << run.consensus_reads << (S == 1 ? " reads" : " read pairs") << " were replaced by their cluster's consensus (FQD_FAST_CONSENSUS=1).\n";
    return true;
}

void HashDupRemover::run_unordered_resident(const std::string* in, const std::string* out)
{
    HIP_OK(hipSetDevice(tuning_.device));
    StreamGuard stream_guard;
    const hipStream_t stream = stream_guard;
    JoinedPairs jp;                                           // (before `eng`: the helper thread makes room in it, and eng's destructor joins that thread first)
    EngineUnderTheRead eng = engine_under_the_read(2, in, tuning_.device, stream, "  on the GPU: engine, key store, table, join arrays (under the read)",
                                                   [&jp](uint64_t reads) { if (reads) jp.prepare(reads); });
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
            if (!cut_records(eng.get()->e, stream, format_, got[s], dev[s])) {             // read it again the host way: that one reports
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
            engine_ok(eng.get()->e, fqd_extract_tags(eng.get()->e, reinterpret_cast<const uint8_t*>(f.text.p), f.start.p, f.id_len.p, f.n, f.tag_off.p, f.tag_len.p));
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
    fqd_engine* engine_now = eng.get()->e;                        // (joins the helper thread: jp is ours from here on)
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
        plan_survivors(eng.get()->e, 2, files, idx, jp.keep.p, upto, gz_out, memlimit_, buffers);
    }

    OutputFile sink0(out[0]), sink1(out[1]);
    OutputFile* sinks[2] = {&sink0, &sink1};

    // ---- outputs: the device assembles windows of survivors in output order, the host writes them -----
    {
        StageClock::Scope t("unordered/resident: survivors out of HBM");
        write_survivors(eng.get()->e, stream, 2, files, idx, jp.keep.p, upto, dups, sinks, format_, memlimit_, true, &buffers);
    }
    if (tuning_.leave_memory_to_exit) g_leave_memory_to_exit = true;
    StageClock::report();
    if (jp.bad) throw_unknown_base(jp.bad_byte);
    summary_.total = n_proc; summary_.duplicates = dups; summary_.unmatched = jp.unmatched;
    if (verbose_) print_unordered_summary(summary_);
}

} // namespace fqdhost
