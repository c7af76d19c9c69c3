// run_sequence.cpp — the sequence-based modes (seq_dup_remover.hpp): every record (pair) to HBM, sorted by sequence and
// compared with its neighbours there, survivors written in sorted order.  The reference sorts before it opens any output
// (seq_dup_remover.hpp:44-50,117-128), so a run that fails on its inputs leaves no output file behind; the same here.
#include "seq_dup_remover.hpp"

#include <fstream>

#include "run_common.hpp"

namespace fqdhost {

using namespace detail;

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
            uint64_t text_bytes = 0;
            if (has_gz_extension(name)) {
                CompressedOnDevice packed;
                if (fetch_bgzf(name, fetch_bytes, device, packed, &f)) ok = finish_on_device(e, stream, format, packed, f);
                else {
                    f.forget();
                    ok = fetch_gzip_ordinary(name, fetch_bytes, device, f, text_bytes) && records_on_device(e, stream, format, text_bytes, f);
                }
            } else ok = fetch_plain(name, fetch_bytes, device, f, text_bytes) && records_on_device(e, stream, format, text_bytes, f);
        } catch (const DeviceOutOfMemory&) { throw; }
        catch (const std::exception&) { ok = false; }
        if (ok) return;
        f.forget();
    }
    hipStream_t up = nullptr;
    HIP_OK(hipStreamCreateWithFlags(&up, hipStreamNonBlocking));
    struct Guard { hipStream_t s; ~Guard() { (void)hipStreamDestroy(s); } } g{up};
    Pinned<uint64_t> h_start, h_seq; Pinned<uint32_t> h_idl, h_sql, h_size;
    Side side;
    side.open_file(name, format, false, block_bytes);
    side.prime(3, device);
    while (side.available() > 0) {
        PooledBlock* b = side.cur;
        const size_t from = side.pos, nb = b->recs.size() - from;
        const RecordRef* r = &b->recs[from];
        const uint64_t text_lo = r[0].start, bytes = r[nb - 1].start + r[nb - 1].size - text_lo;
        f.text.room_for(bytes + 64, up);
        HIP_OK(hipMemcpyAsync(f.text.p + f.text.used, b->text.p + text_lo, bytes, hipMemcpyHostToDevice, up));
        h_start.reserve(nb); h_seq.reserve(nb); h_idl.reserve(nb); h_sql.reserve(nb); h_size.reserve(nb);
        for (size_t k = 0; k < nb; ++k) {
            h_start.p[k] = f.text.used + (r[k].start - text_lo); h_seq.p[k] = h_start.p[k] + r[k].id_len;
            h_idl.p[k] = r[k].id_len; h_sql.p[k] = r[k].seq_len; h_size.p[k] = r[k].size;
        }
        f.start.room_for(nb, up); f.seq_off.room_for(nb, up); f.id_len.room_for(nb, up); f.seq_len.room_for(nb, up); f.size.room_for(nb, up);
        HIP_OK(hipMemcpyAsync(f.start.p + f.n, h_start.p, nb * sizeof(uint64_t), hipMemcpyHostToDevice, up));
        HIP_OK(hipMemcpyAsync(f.seq_off.p + f.n, h_seq.p, nb * sizeof(uint64_t), hipMemcpyHostToDevice, up));
        HIP_OK(hipMemcpyAsync(f.id_len.p + f.n, h_idl.p, nb * sizeof(uint32_t), hipMemcpyHostToDevice, up));
        HIP_OK(hipMemcpyAsync(f.seq_len.p + f.n, h_sql.p, nb * sizeof(uint32_t), hipMemcpyHostToDevice, up));
        HIP_OK(hipMemcpyAsync(f.size.p + f.n, h_size.p, nb * sizeof(uint32_t), hipMemcpyHostToDevice, up));
        HIP_OK(hipStreamSynchronize(up));                    // the block and the staging arrays are reused
        f.text.used += bytes;
        f.start.used = f.seq_off.used = f.id_len.used = f.seq_len.used = f.size.used = f.n + nb;
        f.n += nb;
        side.pos += nb;
    }
    if (side.failed) { std::cerr << side.failure.diag; throw std::runtime_error(side.failure.what); }
}

// `<output>.clusters` (file_utils.cpp:98-112): per sorted record its ID line, "--" in front of the duplicates.  The ID
// lines are gathered in sorted order on the device (fqd_output_plan + fqd_copy_spans) and written as they come back.
void write_clusters(fqd_engine* e, hipStream_t stream, FileOnDevice& f, const uint32_t* perm, const uint8_t* head, uint64_t n,
                    const std::string& name)
{
    auto engine_ok = [&](int rc) { if (rc != FQD_OK) throw std::runtime_error(std::string("GPU engine: ") + fqd_last_error(e)); };
    Device<uint8_t> all; Device<uint64_t> src_off, dst_off; Device<uint32_t> len;
    all.reserve(n); src_off.reserve(n); dst_off.reserve(n + 1); len.reserve(n);
    HIP_OK(hipMemsetAsync(all.p, 1, n, stream));
    uint64_t total = 0;
    engine_ok(fqd_output_plan(e, all.p, perm, n, f.start.p, f.id_len.p, src_off.p, len.p, dst_off.p, &total));
    Device<char> ids; ids.reserve(total + 64);
    engine_ok(fqd_copy_spans(e, reinterpret_cast<const uint8_t*>(f.text.p), src_off.p, len.p, n, reinterpret_cast<uint8_t*>(ids.p), dst_off.p));
    std::vector<char> h_ids(total);
    std::vector<uint32_t> h_len(n);
    std::vector<uint8_t> h_head(n);
    HIP_OK(hipMemcpyAsync(h_ids.data(), ids.p, total, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(h_len.data(), len.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(h_head.data(), head, n, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    std::ofstream out(name, std::ios::binary);
    std::string buf;
    buf.reserve(total + 2 * n);
    uint64_t at = 0;
    for (uint64_t k = 0; k < n; ++k) {
        if (!h_head[k]) buf += "--";
        buf.append(h_ids.data() + at, h_len[k]);
        at += h_len[k];
    }
    out.write(buf.data(), static_cast<std::streamsize>(buf.size()));
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
    for (int s = 0; s < S; ++s) InputFile probe(in[s], true);          // "Cannot open file X" before anything else
    if (tuning_.devices.size() > 1)
        throw std::runtime_error("--compare-seq runs on one GPU: FQD_DEVICES may name one device only");
    const int device = tuning_.devices.size() == 1 ? tuning_.devices[0] : tuning_.device;
    HIP_OK(hipSetDevice(device));
    hipStream_t stream = nullptr;
    HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamDestroy(s); } } sg{stream};
    EngineHandle eng(S, device, stream);
    auto engine_ok = [&](int rc) { if (rc != FQD_OK) throw std::runtime_error(std::string("GPU engine: ") + fqd_last_error(eng.e)); };
    const size_t block_bytes = std::max<size_t>(1u << 20, tuning_.block_bytes);
    const size_t fetch_bytes = std::max<size_t>(block_bytes, 64u << 20);

    FileOnDevice dev[2];
    {
        StageClock::Scope t("sequence: files to HBM, records cut");
        for (int s = 0; s < S; ++s) {
            load_file(eng.e, stream, in[s], format_, device, block_bytes, fetch_bytes, dev[s]);
            if (dev[s].n == 0) throw std::runtime_error("Not enough memory to read a single object!");   // bufferedinput.hpp:81-84
        }
    }
    const uint64_t n = S == 2 ? std::min(dev[0].n, dev[1].n) : dev[0].n;   // pairs end with the shorter file (sort_buckets)
    if (n >= 0x80000000ull) throw std::runtime_error("--compare-seq: at most 2^31-1 records (pairs) per run");
    fqd_tags mates[2];
    for (int s = 0; s < S; ++s)
        mates[s] = fqd_tags{reinterpret_cast<const uint8_t*>(dev[s].text.p), dev[s].seq_off.p, dev[s].seq_len.p, n};
    const fqd_tags* mate2 = S == 2 ? &mates[1] : nullptr;

    Device<uint32_t> perm; Device<uint8_t> head;
    perm.reserve(n); head.reserve(n);
    uint64_t heads = 0;
    {
        StageClock::Scope t("sequence: sort + compare on the GPU");
        engine_ok(fqd_sort_seqs(eng.e, &mates[0], mate2, perm.p));
        engine_ok(fqd_seq_heads(eng.e, &mates[0], mate2, perm.p, static_cast<int>(mode_), distance_, head.p, &heads));
    }
    const uint64_t dups = n - heads;
    FileOnDevice* files[2] = {&dev[0], &dev[1]};
    const uint32_t* idx[2] = {perm.p, perm.p};
    SurvivorBuffers buffers;
    {
        const bool gz_out[2] = {has_gz_extension(out[0]), S == 2 && has_gz_extension(out[1])};
        plan_survivors(eng.e, S, files, idx, head.p, n, gz_out, memlimit_, buffers);
    }
    // outputs exist from here on (the reference opens them after its sort, seq_dup_remover.hpp:58-62,139-146)
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
    if (verbose_) {                                                      // seq_dup_remover.hpp:107-108,216-217
        if (S == 1) std::cout << n << " reads processed, out of which " << dups << " duplicates were removed.\n";
        else        std::cout << n << " read pairs processed, out of which " << dups << " duplicates were removed.\n";
    }
}

} // namespace fqdhost
