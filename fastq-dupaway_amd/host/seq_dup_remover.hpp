// seq_dup_remover.hpp — host driver of the sequence-based modes (`--compare-seq tight|loose|tail-hamming`).
// Same interface as the reference's SeqDupRemover<T> (src/seq_dup_remover.hpp:12-38): filterSE(in, out) and
// filterPE(in1, in2, out1, out2), with the record type as a runtime Format and the comparator as a mode.
// The inputs go to HBM whole (the resident front end of the `--fast` runs: plain, BGZF and ordinary `.gz` inflated on
// the device), are sorted and compared there (fqd_sort_seqs, fqd_seq_heads), and the records that are written leave
// in sorted order through the same writer.  Inputs that do not fit go through HBM in ranges of the sort order (run_ranged;
// FQD_SEQ_RANGE_KB forces it).  FQD_SEQ_KEEP=best writes, of every cluster, the member with the best quality line instead of
// the first in the sort order (fqd_seq_scores, fqd_seq_pick_best).  Limits: one GPU, no sequence byte below '\n'; per range fewer than 2^31 records (pairs)
// and the text and the working set in HBM (`-m` does not bound device memory); a ranged run reads regular files only.
#pragma once
#include <cstdint>
#include <string>
#include <sys/types.h>

#include <hip/hip_runtime_api.h>

#include "hash_dup_remover.hpp"

namespace fqdhost {

enum class CompareSeq { Tight = 0, Loose = 1, Hamming = 2 };   // = FQD_SEQ_TIGHT / _LOOSE / _HAMMING

class SeqDupRemover {
public:
    SeqDupRemover(Format format, ssize_t memlimit, CompareSeq mode, unsigned distance, bool write_clusters, bool verbose,
                  Tuning tuning = Tuning())
        : format_(format), memlimit_(memlimit), mode_(mode), distance_(distance), write_clusters_(write_clusters),
          verbose_(verbose), tuning_(tuning) {}
    void filterSE(const std::string& infile, const std::string& outfile);
    void filterPE(const std::string& infile1, const std::string& infile2, const std::string& outfile1, const std::string& outfile2);
    const Summary& summary() const { return summary_; }
private:
    void run(int n_files, const std::string* in, const std::string* out);
    bool run_in_core(int n_files, const std::string* in, const std::string* out, int device, hipStream_t stream);
    void run_ranged(int n_files, const std::string* in, const std::string* out, int device, hipStream_t stream, uint64_t target_bytes);
    Format     format_;
    ssize_t    memlimit_;
    CompareSeq mode_;
    unsigned   distance_;
    bool       write_clusters_, verbose_;
    bool       keep_best_ = false;       // FQD_SEQ_KEEP=best (read by run(), before any GPU call)
    Tuning     tuning_;
    Summary    summary_;
};

} // namespace fqdhost
