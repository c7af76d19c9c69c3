"""The search mode of the device BGZF coder (FQD_BGZF_SEARCH, fastq-dupaway_amd/csrc/fqd_bgzf_search_core.hpp) on the
CPU: tests/native/bgzf_search_check.cpp runs its functions thread by thread, round by round, as the kernels do.  What it
writes must be BGZF that any gzip reader inflates back to the input, member by member, and it must be SMALLER than what
zlib's deepest greedy level writes member by member.  tests/test_gpu_bgzf_search.py holds the kernels to the same bytes.

Sizes measured with this harness (20 000 records of 150 bases, 7.15 MB; zlib member by member + 26 bytes of framing each):
  fastq_text(20000, 11): fast 2 532 261, high 2 188 067, zlib 3: 2 260 839 (high -3.2 %), zlib 6: 2 130 369 (high +2.7 %)
  binned_text(20000, 3): fast 2 028 877, high 1 743 478, zlib 3: 1 851 414 (high -5.8 %), zlib 6: 1 730 255 (high +0.8 %)"""
import gzip
import time

import pytest

from bgzf_cases import cases, fastq_text
from bgzf_search_cases import FAST, HIGH, all_cases, binned_text, harness_bgzf, zlib_per_member
from test_bgzf_core import EOF_MARK, check_members
from test_bgzf_core import harness_bgzf as fast_harness_bgzf


@pytest.mark.parametrize("name,data,k", list(all_cases()), ids=[c[0] for c in all_cases()])
def test_members_inflate_to_the_input(tmp_path, name, data, k):
    t0 = time.perf_counter()
    raw = harness_bgzf(data, k, HIGH, tmp_path, timeout=120)       # a quadratic search of 160 000 equal prefixes would not come back
    dt = time.perf_counter() - t0
    assert raw.endswith(EOF_MARK)
    assert gzip.decompress(raw) == data
    check_members(raw[:-len(EOF_MARK)], data)                      # every member ALONE: no match reaches into the one before
    if name == "random_bytes":
        assert len(raw) <= len(data) + 31 * 4 + 28
    if name in ("one_symbol", "one_bucket", "period_3", "period_5"):
        assert len(raw) < len(data) // 20
    if name == "one_bucket":
        assert dt < 20.0, dt                                       # bounded work per position: well under a second in fact
    if name == "repeat_beyond_32768":
        assert len(raw) >= len(data)                               # nothing to find within 32768: stored
    if name == "repeat_20000":
        # 80 000 bytes are two members, each on its own: 20 000 + 14 720 random bytes have nothing before them (43 % of
        # the input, a little over 8 bits each), the other 45 280 are some 354 matches of up to 128 bytes
        assert len(raw) < 0.55 * len(data)


@pytest.mark.parametrize("name,data,k", list(cases())[:8], ids=[c[0] for c in list(cases())[:8]])
def test_effort_fast_of_the_new_harness_is_the_fast_coder(tmp_path, name, data, k):
    assert harness_bgzf(data, k, FAST, tmp_path) == fast_harness_bgzf(data, k, tmp_path)


@pytest.mark.parametrize("name,make", [("mixed", lambda: fastq_text(20000, 11)), ("binned", lambda: binned_text(20000, 3))])
def test_high_mode_is_no_larger_than_zlib_3_member_by_member(tmp_path, name, make):
    data = make()
    high = len(harness_bgzf(data, 4, HIGH, tmp_path)) - len(EOF_MARK)
    fast = len(harness_bgzf(data, 4, FAST, tmp_path)) - len(EOF_MARK)
    z3, z6 = zlib_per_member(data, 3), zlib_per_member(data, 6)
    print(f"\n[bgzf search] {name}: {len(data)} bytes -> fast {fast}, high {high}, zlib 3 {z3} ({100 * (high / z3 - 1):+.2f} %), "
          f"zlib 6 {z6} ({100 * (high / z6 - 1):+.2f} %)")
    assert high <= z3, (high, z3)
    assert high < fast, (high, fast)
