// run_sequence.cpp — the sequence-based modes (seq_dup_remover.hpp): every record (pair) to HBM, sorted by sequence and
// compared with its neighbours there, survivors written in sorted order.  The reference sorts before it opens any output
// (seq_dup_remover.hpp:44-50,117-128), so a run that fails on its inputs leaves no output file behind; the same here.
//
// An input that does not fit goes through HBM in RANGES of the sort order (run_ranged below; the rules and their proofs:
// csrc/fqd_seq_range_core.hpp, the memory arithmetic: DESIGN §9): pass A streams the inputs once and keeps a prefix key
// and a size per pair, fqd_seq_plan_ranges cuts the key order into ranges of known size, pass B streams the inputs once
// per range, moves the range's records into a store and runs the same sort, heads and writer on it.
#include "seq_dup_remover.hpp"

#include <cstdio>
#include <cstring>

#include "run_common.hpp"
#include "../csrc/fqd_seq_range_core.hpp"

namespace fqdhost {

using namespace detail;

namespace detail {

// FQD_SEQ_RANGE_KB=N: `--compare-seq` takes the ranged run with N KB of record text per range.  Read here and nowhere else;
// main() asks once before any GPU call, so that a value that is no positive integer ends the run with nothing written.
uint64_t seq_range_target_bytes()
{
    const char* v = std::getenv("FQD_SEQ_RANGE_KB");
    if (!v) return 0;
    uint64_t kb = 0;
    bool ok = *v != 0;
    for (const char* c = v; *c && ok; ++c) {
        if (*c < '0' || *c > '9' || kb > (1ull << 40)) ok = false;
        else kb = kb * 10 + uint64_t(*c - '0');
    }
    if (!ok || kb == 0)
        throw std::runtime_error(std::string("FQD_SEQ_RANGE_KB must be a positive integer (KB of record text per range), not '") + v + "'");
    return kb << 10;
}

// FQD_SEQ_KEEP=first|best: which member of a cluster of duplicates `--compare-seq` writes.  first (and unset): the first in
// the sort order, as the reference's scan does; best: the one with the best quality line (csrc/fqd_seq_pick_core.hpp).
// Read here and nowhere else; SeqDupRemover::run asks before any GPU call.
bool seq_keep_best()
{
    const char* v = std::getenv("FQD_SEQ_KEEP");
    if (!v || std::strcmp(v, "first") == 0) return false;
    if (std::strcmp(v, "best") == 0) return true;
    throw std::runtime_error(std::string("FQD_SEQ_KEEP must be 'first' or 'best', not '") + v + "'");
}

} // namespace detail

namespace {

// A file's records to the tail of f (text, offsets, lengths in HBM) the way the resident runs fetch them: as it lies on
// disk and cut (BGZF / ordinary gzip: inflated too) on the device, or — whatever is irregular — read and cut by the host
// reader, which reports what is wrong in the reference's words.
void load_file(fqd_engine* e, hipStream_t stream, const std::string& name, Format format, int device, size_t block_bytes,
               size_t fetch_bytes, FileOnDevice& f)
{
    if (inflate_on_device()) {
        bool ok = false;
        try {
            Fetched got;
            fetch_file(name, fetch_bytes, device, f, got);
            ok = got.way != Fetched::None && cut_records(e, stream, format, got, f);
        } catch (const DeviceOutOfMemory&) { throw; }
        catch (const std::exception&) { ok = false; }
        if (ok) return;
        f.forget();
    }
    StreamGuard up;
    throw_if_set(append_file(name, format, false, device, block_bytes, f, up));
}

// ---- the ranged run ---------------------------------------------------------------------------------------------------

// A block of the host reader in HBM: its text and, per record, the offsets (from the block's first record) and lengths.
struct BlockOnDevice {
    Device<char> text; Device<uint64_t> start, seq_off; Device<uint32_t> id_len, seq_len, size;
    RecordStaging staging;
    uint64_t bytes = 0;
    void upload(const PooledBlock* b, size_t from, size_t nb, bool with_text, hipStream_t up)
    {
        const RecordRef* r = &b->recs[from];
        const uint64_t text_lo = r[0].start;
        bytes = r[nb - 1].start + r[nb - 1].size - text_lo;
        staging.fill(r, nb, 0);
        start.reserve(nb); seq_off.reserve(nb); id_len.reserve(nb); seq_len.reserve(nb); size.reserve(nb);
        if (with_text) {
            text.reserve(bytes + 64);
            HIP_OK(hipMemcpyAsync(text.p, b->text.p + text_lo, bytes, hipMemcpyHostToDevice, up));
        }
        staging.copy_to(start.p, seq_off.p, id_len.p, seq_len.p, size.p, nb, up);
    }
};

// What a range of `pairs` pairs and `bytes` bytes of record text (both files' together: each store is sized for its own
// file's share, store_bytes below) needs in HBM while it is sorted, compared and written (DESIGN §9a has the derivation):
// the text; per record and file the five arrays of its store (28 B) and the three of the
// output plan (20 B); per pair the order (4 B), the head flags and the heads' scratch (2 B) and the scratch of
// fqd_sort_seqs (64 B and a little); the windows of the writer; with --write-clusters the ID lines (at most the text)
// and their plan (21 B a pair); with FQD_SEQ_KEEP=best the scores (4 B a pair; the pick's own 4 B a pair lie in the scratch
// the sort has left).
uint64_t range_need(int S, uint64_t pairs, uint64_t bytes, bool clusters, bool best, uint64_t writer_bytes)
{
    const uint64_t per_pair = uint64_t(S) * (28u + 20u) + 4u + 2u + 65u + (clusters ? 21u : 0u) + (best ? 4u : 0u);
    return bytes + (clusters ? bytes / 2 : 0) + (pairs + 1) * per_pair + writer_bytes + (64ull << 20);
}

// The two slots of the writer, per file: a window of text and, for a `.gz` output, its members (survivor_writer.cpp).
uint64_t writer_need(int S, const std::string* out, long long memlimit)
{
    uint64_t window = std::max<uint64_t>(4u << 20, static_cast<uint64_t>(memlimit > 0 ? memlimit : (2ll << 30)) / 16);
    if (const char* v = std::getenv("FQD_STREAM_WINDOW_KB")) { const long kb = std::atol(v); if (kb > 0) window = static_cast<uint64_t>(kb) << 10; }
    const uint64_t roomy = window + window / 4;
    uint64_t all = 0;
    for (int s = 0; s < S; ++s) all += 2 * (roomy + 64 + (has_gz_extension(out[s]) && deflate_on_device() ? fqd_bgzf_bound(roomy) : 0));
    return all;
}

// The bytes of file s's records in a range (the plan keeps the first file's share of a pair's bytes).
uint64_t store_bytes(const fqd_seq_range& r, int S, int s)
{
    return S == 1 ? r.bytes : s == 0 ? r.bytes_mate1 : r.bytes - r.bytes_mate1;
}

std::string show_prefix(uint64_t key)
{
    std::string t;
    for (int j = 7; j >= 0; --j) {
        const unsigned c = unsigned(key >> (8 * j)) & 255u;
        if (c == '\n') break;
        if (c >= 0x20 && c < 0x7F) t += static_cast<char>(c);
        else { char h[8]; std::snprintf(h, sizeof h, "\\x%02X", c); t += h; }
    }
    return t;
}

// The record (pair) the comparator holds when it leaves a range (fqd_seq_range_core.hpp): whole text and lengths.
struct Carry {
    bool set = false;
    Device<char> text[2]; uint32_t id_len[2] = {0, 0}, seq_len[2] = {0, 0}, size[2] = {0, 0};
};

uint64_t peek_u64(const uint64_t* d, uint64_t k, hipStream_t s)
{
    uint64_t v = 0;
    HIP_OK(hipMemcpyAsync(&v, d + k, sizeof v, hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return v;
}

} // namespace

void SeqDupRemover::filterSE(const std::string& infile, const std::string& outfile)
{
    const std::string in[1] = {infile}, out[1] = {outfile};
    try { run(1, in, out); }
    catch (const DiagnosedError& e) { std::cerr << e.diag; throw; }
}

void SeqDupRemover::filterPE(const std::string& infile1, const std::string& infile2, const std::string& outfile1, const std::string& outfile2)
{
    const std::string in[2] = {infile1, infile2}, out[2] = {outfile1, outfile2};
    try { run(2, in, out); }
    catch (const DiagnosedError& e) { std::cerr << e.diag; throw; }
}

void SeqDupRemover::run(int S, const std::string* in, const std::string* out)
{
    keep_best_ = seq_keep_best();                                       // a misspelt FQD_SEQ_KEEP ends the run before any GPU call
    if (keep_best_ && format_ == Format::Fasta)
        throw std::runtime_error("FQD_SEQ_KEEP=best needs the quality lines of FASTQ records: --format fasta has none");
    for (int s = 0; s < S; ++s) InputFile probe(in[s], true);          // "Cannot open file X" before anything else
    if (tuning_.devices.size() > 1)
        throw std::runtime_error("--compare-seq runs on one GPU: FQD_DEVICES may name one device only");
    const int device = tuning_.devices.size() == 1 ? tuning_.devices[0] : tuning_.device;
    HIP_OK(hipSetDevice(device));
    StreamGuard stream;

    // In core unless FQD_SEQ_RANGE_KB asks for ranges, plain inputs are plainly too large for the free HBM (their text and
    // two fifths of it again for the working set: what range_need comes to for records of 300 bytes), or the in-core
    // load runs out of HBM — which it does before any output exists.
    uint64_t target = seq_range_target_bytes();
    bool ranged = target != 0;
    if (!ranged) {
        uint64_t text = 0, size = 0;
        bool plain = true;
        for (int s = 0; s < S; ++s) { if (has_gz_extension(in[s]) || !is_regular_file(in[s], size)) plain = false; else text += size; }
        size_t free_b = 0, total_b = 0;
        HIP_OK(hipMemGetInfo(&free_b, &total_b));
        ranged = plain && text + text / 5 * 2 > free_b;
    }
    if (!ranged && run_in_core(S, in, out, device, stream)) return;
    run_ranged(S, in, out, device, stream, target);
}

// Everything in HBM at once.  false: HBM ran out, or the inputs hold 2^31 records (pairs) or more, before an output existed;
// everything is released again and the run goes on in ranges.
bool SeqDupRemover::run_in_core(int S, const std::string* in, const std::string* out, int device, hipStream_t stream)
{
    bool outputs_exist = false;
    try {
    EngineHandle eng(S, device, stream);
    const size_t block_bytes = block_bytes_for(tuning_, 0), fetch_bytes = fetch_bytes_for(block_bytes, 0);   // (no --mem-limit term here)

    FileOnDevice dev[2];
    {
        StageClock::Scope t("sequence: files to HBM, records cut");
        for (int s = 0; s < S; ++s) {
            load_file(eng.e, stream, in[s], format_, device, block_bytes, fetch_bytes, dev[s]);
            if (dev[s].n == 0) throw std::runtime_error("Not enough memory to read a single object!");   // bufferedinput.hpp:81-84
        }
    }
    const uint64_t n = S == 2 ? std::min(dev[0].n, dev[1].n) : dev[0].n;   // pairs end with the shorter file (sort_buckets)
    if (n >= 0x80000000ull) return false;   // the sort takes fewer than 2^31 records (pairs): in ranges, then (nothing is written yet)
    fqd_tags mates[2];
    for (int s = 0; s < S; ++s)
        mates[s] = fqd_tags{reinterpret_cast<const uint8_t*>(dev[s].text.p), dev[s].seq_off.p, dev[s].seq_len.p, n};
    const fqd_tags* mate2 = S == 2 ? &mates[1] : nullptr;

    Device<uint32_t> perm; Device<uint8_t> head;
    perm.reserve(n); head.reserve(n);
    uint64_t heads = 0;
    {
        StageClock::Scope t("sequence: sort + compare on the GPU");
        engine_ok(eng.e, fqd_sort_seqs(eng.e, &mates[0], mate2, perm.p));
        engine_ok(eng.e, fqd_seq_heads(eng.e, &mates[0], mate2, perm.p, static_cast<int>(mode_), distance_, head.p, &heads));
    }
    const uint64_t dups = n - heads;
    FileOnDevice* files[2] = {&dev[0], &dev[1]};
    if (keep_best_) {
        const uint64_t moved = pick_best_members(eng.e, S, files, n, head.p, perm.p);
        if (StageClock::on()) std::cerr << "sequence: best-quality pick, " << moved << " of " << heads << " clusters changed\n";
    }
    const uint32_t* idx[2] = {perm.p, perm.p};
    SurvivorBuffers buffers;
    {
        const bool gz_out[2] = {has_gz_extension(out[0]), S == 2 && has_gz_extension(out[1])};
        plan_survivors(eng.e, S, files, idx, head.p, n, gz_out, memlimit_, buffers);
    }
    // outputs exist from here on (the reference opens them after its sort, seq_dup_remover.hpp:58-62,139-146)
    outputs_exist = true;
    OutputFile sink0(out[0]);
    std::unique_ptr<OutputFile> sink1;
    if (S == 2) sink1 = std::make_unique<OutputFile>(out[1]);
    OutputFile* sinks[2] = {&sink0, sink1.get()};
    if (write_clusters_)
        for (int s = 0; s < S; ++s) write_clusters(eng.e, stream, dev[s], perm.p, head.p, n, out[s] + ".clusters");
    {
        StageClock::Scope t("sequence: survivors out of HBM");
        write_survivors(eng.e, stream, S, files, idx, head.p, n, dups, sinks, format_, memlimit_, true, &buffers);
    }
    if (tuning_.leave_memory_to_exit) g_leave_memory_to_exit = true;
    StageClock::report();
    summary_.total = n; summary_.duplicates = dups; summary_.unmatched = 0;
    if (verbose_) print_summary(S, n, dups);
    return true;
    } catch (const DeviceOutOfMemory&) {
        if (outputs_exist) throw;
        return false;                                    // the engine, the text and every buffer above are released by now
    }
}

// The inputs through HBM in ranges of the sort order.  target = 0: what the free HBM allows.
void SeqDupRemover::run_ranged(int S, const std::string* in, const std::string* out, int device, hipStream_t stream, uint64_t target)
{
    for (int s = 0; s < S; ++s) {
        uint64_t size = 0;
        if (!is_regular_file(in[s], size))
            throw std::runtime_error("--compare-seq: the input does not fit in GPU memory at once (or FQD_SEQ_RANGE_KB is set) and is then read "
                                     "once per range of the sort order, which a pipe cannot be: " + in[s] + " is not a regular file");
    }
    // A loose or tail-hamming cluster can go on behind a cut (through the carried record), and the range in front of the
    // cut is on disk by the time its later members are seen: the best member of such a cluster cannot take its place.
    if (keep_best_ && mode_ != CompareSeq::Tight)
        throw std::runtime_error("FQD_SEQ_KEEP=best with --compare-seq loose or tail-hamming needs the whole input in GPU memory at once; "
                                 "this run goes through it in ranges of the sort order (FQD_SEQ_RANGE_KB is set, or the input does not fit)");
    const size_t block_bytes = block_bytes_for(tuning_, 0);
    BlockOnDevice blk;
    Device<uint32_t> range_of;
    std::vector<fqd_seq_range> table;
    uint64_t n = 0;

    {   // ---- pass A: a key and a size per pair; everything that can refuse the run, before any output exists ----
        StageClock::Scope t("sequence: pass A, keys and sizes of every pair");
        EngineHandle eng(S, device, stream);
        GrowDevice<uint64_t> key; GrowDevice<uint32_t> bytes, bytes0;     // bytes0: the first file's part of a pair's bytes
        uint64_t count[2] = {0, 0}, first_with[10], record_bytes = 0;
        for (uint64_t& f : first_with) f = ~0ull;
        for (int s = 0; s < S; ++s) {
            throw_if_set(stream_blocks(in[s], format_, false, device, block_bytes, [&](const PooledBlock* b, size_t from, size_t nb, uint64_t base) {
                count[s] = base + nb;
                // the second file's records beyond the first file's have no partner: they are counted, nothing else
                const uint64_t take = s == 0 ? nb : (base < count[0] ? std::min<uint64_t>(nb, count[0] - base) : 0);
                if (take == 0) return;
                blk.upload(b, from, take, true, stream);
                if (s == 0) {
                    try { key.room_for(take, stream); bytes.room_for(take, stream); if (S == 2) bytes0.room_for(take, stream); }
                    catch (const DeviceOutOfMemory&) { throw DeviceOutOfMemory("--compare-seq: GPU memory ran out while the keys of the pairs were collected (12 to 16 bytes a pair)"); }
                }
                const fqd_tags tags{reinterpret_cast<const uint8_t*>(blk.text.p), blk.seq_off.p, blk.seq_len.p, take};
                fqd_seq_block_info info;
                engine_ok(eng.e, fqd_seq_prefix_keys(eng.e, &tags, nullptr, blk.size.p, nullptr, s == 1, s == 0 ? key.p + base : nullptr,
                                              bytes.p + base, &info));                          // waits for the stream: the block is free again
                if (s == 0) {
                    if (S == 2) {
                        HIP_OK(hipMemcpyAsync(bytes0.p + base, bytes.p + base, take * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
                        HIP_OK(hipStreamSynchronize(stream));
                        bytes0.used += take;
                    }
                    key.used += take; bytes.used += take;
                }
                for (int c = 0; c < 10; ++c) if (info.first_with[c] != ~0ull) first_with[c] = std::min(first_with[c], base + info.first_with[c]);
                record_bytes += info.record_bytes;
            }));
            if (count[s] == 0) throw std::runtime_error("Not enough memory to read a single object!");   // bufferedinput.hpp:81-84
        }
        n = S == 2 ? std::min(count[0], count[1]) : count[0];              // pairs end with the shorter file (sort_buckets)
        for (unsigned c = 0; c < 10; ++c)
            if (first_with[c] < n) {                                         // what the census of fqd_sort_seqs says of the same records
                char msg[200];
                std::snprintf(msg, sizeof msg, FQD_SEQ_LOW_BYTE_FORMAT, c);
                throw std::runtime_error(std::string("GPU engine: ") + msg);
            }
        if (n >= 0x100000000ull) throw std::runtime_error("--compare-seq: at most 2^32-1 records (pairs) per run");
        const bool auto_target = target == 0;
        const uint64_t writer_bytes = writer_need(S, out, memlimit_);
        if (auto_target) {
            // the largest range whose need (range_need, with the input's own bytes per pair) stays within four fifths of what
            // is free once the plan's scratch (24 B a pair, released before pass B) and the range numbers (4 B) are there
            size_t free_b = 0, total_b = 0;
            HIP_OK(hipMemGetInfo(&free_b, &total_b));
            const uint64_t fixed = range_need(S, 0, 0, write_clusters_, keep_best_, writer_bytes) + n * 4u;
            const uint64_t usable = free_b / 5 * 4;
            if (usable <= fixed) throw DeviceOutOfMemory("--compare-seq: too little GPU memory is free for the ranged run");
            const double per_byte = double(range_need(S, n, record_bytes, write_clusters_, keep_best_, writer_bytes) - range_need(S, 0, 0, write_clusters_, keep_best_, writer_bytes)) /
                                    double(std::max<uint64_t>(record_bytes, 1));
            target = std::max<uint64_t>(1u << 20, static_cast<uint64_t>(double(usable - fixed) / per_byte));
            // and few enough pairs a range for the sort (fewer than 2^31): 2^30 of the input's average pair
            target = std::min<uint64_t>(target, std::max<uint64_t>(1u << 20, record_bytes / n * (1ull << 30)));
        }
        range_of.reserve(n);
        uint32_t R = 0, room = 4096;
        for (;;) {
            table.resize(room);
            engine_ok(eng.e, fqd_seq_plan_ranges(eng.e, key.p, bytes.p, S == 2 ? bytes0.p : nullptr, n, target, range_of.p, table.data(), room, &R));
            if (R <= room) break;
            room = R;
        }
        table.resize(R);
    }   // the keys, the sizes and the plan's scratch are released here

    uint64_t largest = 0;
    for (const fqd_seq_range& r : table) largest = std::max(largest, r.bytes);
    if (StageClock::on()) std::cerr << "sequence: ranged run, " << table.size() << " ranges, largest " << largest << " bytes\n";
    {   // every range's need against the free HBM, before any output exists
        size_t free_b = 0, total_b = 0;
        HIP_OK(hipMemGetInfo(&free_b, &total_b));
        const uint64_t writer_bytes = writer_need(S, out, memlimit_);
        for (const fqd_seq_range& r : table) {
            if (r.pairs + 1 >= 0x80000000ull)
                throw std::runtime_error("--compare-seq: at most 2^31-2 records (pairs) per range; the sequences that start with '" +
                                         show_prefix(r.key_lo) + "' to '" + show_prefix(r.key_hi) + "' are " + std::to_string(r.pairs));
            const uint64_t need = range_need(S, r.pairs, r.bytes, write_clusters_, keep_best_, writer_bytes);
            if (need > free_b)
                throw std::runtime_error("--compare-seq: the records whose sequence starts with '" + show_prefix(r.key_lo) +
                                         (r.key_hi != r.key_lo ? "' to '" + show_prefix(r.key_hi) : std::string()) + "' are " + std::to_string(r.bytes) +
                                         " bytes in " + std::to_string(r.pairs) + " records (pairs): sorting them needs about " + std::to_string(need >> 20) +
                                         " MiB of GPU memory and " + std::to_string(free_b >> 20) + " MiB are free");
        }
    }

    // ---- pass B: range after range ----
    EngineHandle eng(S, device, stream);
    const bool carries = mode_ != CompareSeq::Tight;          // tight: nothing crosses a cut (fqd_seq_range_core.hpp)
    Carry carry;
    FileOnDevice store[2];
    Device<uint8_t> keep; Pinned<uint8_t> h_keep;
    Device<uint64_t> src_off, dst_off; Device<uint32_t> len;
    Pinned<uint64_t> c_start, c_seq; Pinned<uint32_t> c_idl, c_sql, c_size;
    Device<uint32_t> perm; Device<uint8_t> head;
    SurvivorBuffers buffers;
    std::unique_ptr<OutputFile> sink[2];
    OutputFile* sinks[2] = {nullptr, nullptr};
    const bool gz_out[2] = {has_gz_extension(out[0]), S == 2 && has_gz_extension(out[1])};
    uint64_t total = 0, total_dups = 0, moved_clusters = 0, all_clusters = 0;
    std::vector<uint8_t> tail;

    // The stores, the order and the flags for the LARGEST range, before any output exists: a later, larger range must not be
    // what runs out of HBM.  (The scratch of the sort and the writer's windows still grow with the ranges; range_need has
    // held every range against the free memory above.)
    constexpr uint64_t kCarryRoom = 1u << 20;
    auto store_room = [&](auto& g, uint64_t count) {
        try { g.room_for(count, stream); }
        catch (const DeviceOutOfMemory&) { throw DeviceOutOfMemory("--compare-seq: GPU memory ran out while the store of a range was made"); }
    };
    {
        uint64_t most_pairs = 0, most_text[2] = {0, 0};
        for (const fqd_seq_range& r : table) {
            most_pairs = std::max(most_pairs, r.pairs + 1);
            for (int s = 0; s < S; ++s) most_text[s] = std::max(most_text[s], store_bytes(r, S, s));
        }
        for (int s = 0; s < S; ++s) {
            FileOnDevice& f = store[s];
            store_room(f.text, most_text[s] + kCarryRoom + 64);
            store_room(f.start, most_pairs); store_room(f.seq_off, most_pairs); store_room(f.id_len, most_pairs);
            store_room(f.seq_len, most_pairs); store_room(f.size, most_pairs);
        }
        perm.reserve(most_pairs); head.reserve(most_pairs);
    }

    for (uint32_t r = 0; r < table.size(); ++r) {
        const uint64_t phantom = carry.set ? 1 : 0, want = table[r].pairs + phantom;
        {
            StageClock::Scope t("sequence: pass B, a range's records to its store");
            for (int s = 0; s < S; ++s) {
                FileOnDevice& f = store[s];
                f.forget();
                // sized before the first range, for the largest one; only a carried record of more than kCarryRoom bytes grows it
                const uint64_t text_room = store_bytes(table[r], S, s) + (carry.set ? carry.size[s] : 0) + 64;
                if (f.text.cap < text_room) { f.text.release(); store_room(f.text, text_room); }
                if (carry.set) {                                 // the phantom: record 0, whole text
                    const uint64_t at0 = 0, seq0 = carry.id_len[s];
                    HIP_OK(hipMemcpyAsync(f.text.p, carry.text[s].p, carry.size[s], hipMemcpyDeviceToDevice, stream));
                    HIP_OK(hipMemcpyAsync(f.start.p, &at0, sizeof at0, hipMemcpyHostToDevice, stream));
                    HIP_OK(hipMemcpyAsync(f.seq_off.p, &seq0, sizeof seq0, hipMemcpyHostToDevice, stream));
                    HIP_OK(hipMemcpyAsync(f.id_len.p, &carry.id_len[s], sizeof(uint32_t), hipMemcpyHostToDevice, stream));
                    HIP_OK(hipMemcpyAsync(f.seq_len.p, &carry.seq_len[s], sizeof(uint32_t), hipMemcpyHostToDevice, stream));
                    HIP_OK(hipMemcpyAsync(f.size.p, &carry.size[s], sizeof(uint32_t), hipMemcpyHostToDevice, stream));
                    HIP_OK(hipStreamSynchronize(stream));
                    f.text.used = carry.size[s]; f.n = 1;
                }
                throw_if_set(stream_blocks(in[s], format_, false, device, block_bytes, [&](const PooledBlock* b, size_t from, size_t nb, uint64_t base) {
                    if (base >= n) return;                       // behind the last pair
                    const uint64_t take = std::min<uint64_t>(nb, n - base);
                    keep.reserve(take);
                    uint64_t kept = 0, moved = 0;
                    engine_ok(eng.e, fqd_range_keep(eng.e, range_of.p + base, take, r, keep.p, &kept));
                    if (kept == 0) return;
                    if (f.n + kept > want) throw std::runtime_error("--compare-seq: an input changed between the passes of the ranged run");
                    blk.upload(b, from, take, true, stream);
                    src_off.reserve(take); dst_off.reserve(take + 1); len.reserve(take);
                    engine_ok(eng.e, fqd_output_plan(eng.e, keep.p, nullptr, take, blk.start.p, blk.size.p, src_off.p, len.p, dst_off.p, &moved));
                    if (f.text.used + moved + 64 > f.text.cap) throw std::runtime_error("--compare-seq: an input changed between the passes of the ranged run");
                    engine_ok(eng.e, fqd_copy_spans(eng.e, reinterpret_cast<const uint8_t*>(blk.text.p), src_off.p, len.p, take,
                                             reinterpret_cast<uint8_t*>(f.text.p) + f.text.used, dst_off.p));
                    // the kept records' places in the store, in input order (what fqd_output_plan's dst_off says, re-based)
                    h_keep.reserve(take);
                    HIP_OK(hipMemcpyAsync(h_keep.p, keep.p, take, hipMemcpyDeviceToHost, stream));
                    HIP_OK(hipStreamSynchronize(stream));
                    c_start.reserve(kept); c_seq.reserve(kept); c_idl.reserve(kept); c_sql.reserve(kept); c_size.reserve(kept);
                    const RecordRef* rec = &b->recs[from];
                    uint64_t at = f.text.used, j = 0;
                    for (uint64_t k = 0; k < take; ++k) {
                        if (!h_keep.p[k]) continue;
                        c_start.p[j] = at; c_seq.p[j] = at + rec[k].id_len;
                        c_idl.p[j] = rec[k].id_len; c_sql.p[j] = rec[k].seq_len; c_size.p[j] = rec[k].size;
                        at += rec[k].size; ++j;
                    }
                    HIP_OK(hipMemcpyAsync(f.start.p + f.n, c_start.p, kept * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
                    HIP_OK(hipMemcpyAsync(f.seq_off.p + f.n, c_seq.p, kept * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
                    HIP_OK(hipMemcpyAsync(f.id_len.p + f.n, c_idl.p, kept * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
                    HIP_OK(hipMemcpyAsync(f.seq_len.p + f.n, c_sql.p, kept * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
                    HIP_OK(hipMemcpyAsync(f.size.p + f.n, c_size.p, kept * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
                    HIP_OK(hipStreamSynchronize(stream));        // the block and the staging arrays are reused
                    f.text.used = at; f.n += kept;
                }));
                f.start.used = f.seq_off.used = f.id_len.used = f.seq_len.used = f.size.used = f.n;
                if (f.n != want) throw std::runtime_error("--compare-seq: an input changed between the passes of the ranged run");
            }
        }
        const uint64_t m = want;                                 // records of the store, the phantom included
        fqd_tags mates[2];
        for (int s = 0; s < S; ++s)
            mates[s] = fqd_tags{reinterpret_cast<const uint8_t*>(store[s].text.p), store[s].seq_off.p, store[s].seq_len.p, m};
        const fqd_tags* mate2 = S == 2 ? &mates[1] : nullptr;
        perm.reserve(m); head.reserve(m);
        uint64_t heads = 0;
        {
            StageClock::Scope t("sequence: sort + compare on the GPU");
            engine_ok(eng.e, fqd_sort_seqs(eng.e, &mates[0], mate2, perm.p));
            if (phantom && peek_u32(perm.p, 0, stream) != 0) throw std::runtime_error("--compare-seq: internal error (the carried record is not the first of its range)");
            engine_ok(eng.e, fqd_seq_heads(eng.e, &mates[0], mate2, perm.p, static_cast<int>(mode_), distance_, head.p, &heads));
            if (phantom) {                                       // written, listed and counted in its own range
                HIP_OK(hipMemsetAsync(head.p, 0, 1, stream));
                HIP_OK(hipStreamSynchronize(stream));
                heads -= 1;
            }
        }
        const uint64_t dups = (m - phantom) - heads;
        FileOnDevice* files[2] = {&store[0], &store[1]};
        if (keep_best_) {                                        // tight only: no phantom, and no cluster crosses a cut
            moved_clusters += pick_best_members(eng.e, S, files, m, head.p, perm.p);
            all_clusters += heads;
        }
        const uint32_t* idx[2] = {perm.p, perm.p};
        plan_survivors(eng.e, S, files, idx, head.p, m, gz_out, memlimit_, buffers);
        if (r == 0) {                                            // outputs exist from here on
            for (int s = 0; s < S; ++s) { sink[s] = std::make_unique<OutputFile>(out[s]); sinks[s] = sink[s].get(); }
        }
        if (write_clusters_)
            for (int s = 0; s < S; ++s)
                write_clusters(eng.e, stream, store[s], perm.p + phantom, head.p + phantom, m - phantom, out[s] + ".clusters", r > 0);
        {
            StageClock::Scope t("sequence: survivors out of HBM");
            write_survivors(eng.e, stream, S, files, idx, head.p, m, m - heads, sinks, format_, memlimit_, false, &buffers);
        }
        total += m - phantom; total_dups += dups;

        if (carries && r + 1 < table.size()) {
            // loose: the last sorted record; tail-hamming: the last head (none: the carried record stays)
            uint64_t at = m - 1;
            bool found = true;
            if (mode_ == CompareSeq::Hamming) {
                found = false;
                for (uint64_t hi = m; hi > 0 && !found;) {
                    const uint64_t lo = hi > 65536 ? hi - 65536 : 0;
                    tail.resize(hi - lo);
                    HIP_OK(hipMemcpyAsync(tail.data(), head.p + lo, hi - lo, hipMemcpyDeviceToHost, stream));
                    HIP_OK(hipStreamSynchronize(stream));
                    for (uint64_t k = hi; k > lo; --k) if (tail[k - 1 - lo]) { at = k - 1; found = true; break; }
                    hi = lo;
                }
            }
            if (found) {
                const uint32_t rec = peek_u32(perm.p, at, stream);
                for (int s = 0; s < S; ++s) {
                    const uint64_t from = peek_u64(store[s].start.p, rec, stream);
                    carry.id_len[s] = peek_u32(store[s].id_len.p, rec, stream);
                    carry.seq_len[s] = peek_u32(store[s].seq_len.p, rec, stream);
                    carry.size[s] = peek_u32(store[s].size.p, rec, stream);
                    // (never the phantom's own text: that record is `found` only when it is not the carried one)
                    Device<char> next;
                    next.reserve(carry.size[s] + 64);
                    HIP_OK(hipMemcpyAsync(next.p, store[s].text.p + from, carry.size[s], hipMemcpyDeviceToDevice, stream));
                    HIP_OK(hipStreamSynchronize(stream));
                    std::swap(carry.text[s].p, next.p); std::swap(carry.text[s].cap, next.cap);
                }
                carry.set = true;
            }
        }
    }
    for (int s = 0; s < S; ++s) sinks[s]->close();
    if (tuning_.leave_memory_to_exit) g_leave_memory_to_exit = true;
    if (keep_best_ && StageClock::on())
        std::cerr << "sequence: best-quality pick, " << moved_clusters << " of " << all_clusters << " clusters changed\n";
    StageClock::report();
    summary_.total = total; summary_.duplicates = total_dups; summary_.unmatched = 0;
    if (verbose_) print_summary(S, total, total_dups);
}

} // namespace fqdhost
