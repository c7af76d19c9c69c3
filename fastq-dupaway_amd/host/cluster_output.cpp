// cluster_output.cpp — what the runs that know whole clusters share (run_sequence.cpp: `--compare-seq`; run_resident.cpp:
// `--fast` with FQD_FAST_KEEP / FQD_FAST_CLUSTERS): the `<output>.clusters` file from an order and its head flags, and the
// best-quality member of every cluster put at the head's place of the order.
#include <fstream>

#include "run_common.hpp"

namespace fqdhost {
namespace detail {

// The text of `<output>.clusters` (file_utils.cpp:98-112): per record of the order its ID line, "--" in front of the
// members that are not written.  The ID lines are gathered in that order on the device (fqd_output_plan +
// fqd_copy_spans); everything the device and the host need for it is allocated and released in here, so a run can
// call this BEFORE it creates an output.
std::string cluster_lines(fqd_engine* e, hipStream_t stream, FileOnDevice& f, const uint32_t* perm, const uint8_t* head, uint64_t n)
{
    Device<uint8_t> all; Device<uint64_t> src_off, dst_off; Device<uint32_t> len;
    all.reserve(n); src_off.reserve(n); dst_off.reserve(n + 1); len.reserve(n);
    HIP_OK(hipMemsetAsync(all.p, 1, n, stream));
    uint64_t total = 0;
    engine_ok(e, fqd_output_plan(e, all.p, perm, n, f.start.p, f.id_len.p, src_off.p, len.p, dst_off.p, &total));
    Device<char> ids; ids.reserve(total + 64);
    engine_ok(e, fqd_copy_spans(e, reinterpret_cast<const uint8_t*>(f.text.p), src_off.p, len.p, n, reinterpret_cast<uint8_t*>(ids.p), dst_off.p));
    std::vector<char> h_ids(total);
    std::vector<uint32_t> h_len(n);
    std::vector<uint8_t> h_head(n);
    HIP_OK(hipMemcpyAsync(h_ids.data(), ids.p, total, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(h_len.data(), len.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipMemcpyAsync(h_head.data(), head, n, hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    std::string buf;
    buf.reserve(total + 2 * n);
    uint64_t at = 0;
    for (uint64_t k = 0; k < n; ++k) {
        if (!h_head[k]) buf += "--";
        buf.append(h_ids.data() + at, h_len[k]);
        at += h_len[k];
    }
    return buf;
}

void write_cluster_lines(const std::string& lines, const std::string& name, bool append)
{
    std::ofstream out(name, append ? std::ios::binary | std::ios::app : std::ios::binary);
    out.write(lines.data(), static_cast<std::streamsize>(lines.size()));
}

void write_clusters(fqd_engine* e, hipStream_t stream, FileOnDevice& f, const uint32_t* perm, const uint8_t* head, uint64_t n,
                    const std::string& name, bool append)
{
    write_cluster_lines(cluster_lines(e, stream, f, perm, head, n), name, append);
}

// Per cluster of `head` the member with the best quality line takes the head's place in `perm` (fqd_seq_scores over
// the whole records of the n pairs, fqd_seq_pick_best); everything after it reads perm as before.
// Returns the number of clusters whose written member changed.
uint64_t pick_best_members(fqd_engine* e, int S, FileOnDevice* const* files, uint64_t n, const uint8_t* head, uint32_t* perm, const char* stage)
{
    StageClock::Scope t(stage);
    fqd_tags recs[2];
    for (int s = 0; s < S; ++s)
        recs[s] = fqd_tags{reinterpret_cast<const uint8_t*>(files[s]->text.p), files[s]->start.p, files[s]->size.p, n};
    Device<uint32_t> score;
    score.reserve(n);
    uint64_t moved = 0;
    engine_ok(e, fqd_seq_scores(e, &recs[0], S == 2 ? &recs[1] : nullptr, score.p));
    engine_ok(e, fqd_seq_pick_best(e, score.p, head, n, perm, &moved));
    return moved;
}

// `<output 1>.duplevels`: a header, the sixteen levels of csrc/fqd_size_core.hpp (all always there), the totals and the
// largest cluster, tab-separated.
std::string duplevels_text(const fqd_size_levels& lv)
{
    static const char* const kRows[16] = {"1", "2", "3", "4", "5", "6", "7", "8", "9", "10-49", "50-99", "100-499", "500-999", "1000-4999", "5000-9999", "10000+"};
    std::string text = "#level\tclusters\trecords\n";
    uint64_t clusters = 0, records = 0;
    for (int k = 0; k < 16; ++k) {
        text += std::string(kRows[k]) + "\t" + std::to_string(lv.clusters[k]) + "\t" + std::to_string(lv.records[k]) + "\n";
        clusters += lv.clusters[k]; records += lv.records[k];
    }
    text += "#total\t" + std::to_string(clusters) + "\t" + std::to_string(records) + "\n";
    text += "#largest\t" + std::to_string(lv.largest) + "\n";
    return text;
}

} // namespace detail
} // namespace fqdhost
