"""The record arrays of a text by the host scanner's rule, in plain numpy: the yardstick of fqd_scan_records
(csrc/fqd_inflate.hip) in tests/test_gpu_inflate.py and tests/test_gpu_scan_edges.py.

The reference is nothing but the positions of '\\n', taken K at a time (K = 4 for FASTQ, 2 for FASTA)."""
import numpy as np


def numpy_records(data: bytes, k: int):
    nl = np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10)
    n = len(nl) // k
    ends = nl[: n * k].reshape(n, k)
    start = np.concatenate([[0], ends[:-1, -1] + 1]) if n else np.zeros(0, np.int64)
    return start, ends[:, 0] + 1, ends[:, 0] - start + 1, ends[:, 1] - ends[:, 0] - 1, ends[:, -1] - start + 1
