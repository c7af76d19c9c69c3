/* fqdupaway.h — C ABI of the MI355X-native `--fast` deduplication engine.
 *
 * The reference (fastq-dupaway V1.5.0) has no FFI: its seam for this path is the
 * C++ class template HashDupRemover<T> (src/hash_dup_remover.hpp:73-94), which
 * builds one key per record (setRecord / setRecordPair, hpp:19-41 via
 * SeqUtils::seq2hash, src/seq_utils.cpp:35-49) and runs find-then-insert on a
 * std::unordered_set (hpp:70-71,126-144,228-248).  This header is what a
 * binding for that loop would call instead: the host side keeps parsing
 * records and writing survivors (fastq-dupaway_amd/host mirrors
 * HashDupRemover's constructor, filterSE and filterPE), and hands batches of
 * sequences to the device, which answers with one keep flag per record.
 *
 * Conventions: plain pointers and sizes only; every function returns an int
 * status (FQD_OK = 0) and never throws; the text of the last failure of an
 * engine is available from fqd_last_error().  `device` pointers are HIP
 * device pointers, `stream` is a hipStream_t passed as void*.
 *
 * Buffers: no entry point reads or writes a caller's buffer outside the extent stated at its declaration (n entries,
 * the bytes a span or an offset array names, a capacity), and a `const` input comes back bit for bit; what lies before
 * or behind a buffer, and where it lies — offsets into a text may exceed 2^32 — changes no result.  (Byte buffers are
 * loaded in aligned words of up to 16 bytes, so a load may cover the rest of the aligned 16 bytes that hold a buffer's
 * first or last byte; such a word never crosses a page, and none of those bytes reaches a result.  Stores are exact.)
 * A pointer needs the natural alignment of its element type (uint32_t: 4, uint64_t: 8, bytes: none) and no more,
 * unless its declaration says otherwise.  The one exception written down: fqd_gunzip / fqd_gunzip_arriving want 32
 * readable bytes behind the last byte of the packed input.  (tests/test_gpu_buffer_extents.py holds every entry point
 * to this.)
 *
 * Contract: record i of an engine's input
 * order is KEPT iff no record j < i has the identical sequence (for paired
 * engines: identical mate-1 AND mate-2 sequences, lengths included) over the
 * alphabet {A,C,G,T,N}.  Selection is exact — hashes only place keys — and
 * the first occurrence always wins.  Any other byte is an error that carries
 * the offending byte, as SeqUtils::_char2number does (seq_utils.cpp:3-21).
 */
#ifndef FQDUPAWAY_H
#define FQDUPAWAY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FQD_ABI_VERSION 5

/* status codes */
#define FQD_OK              0
#define FQD_ERR_ARG         1   /* bad argument / misuse                              */
#define FQD_ERR_HIP         2   /* a HIP runtime call failed (see fqd_last_error)     */
#define FQD_ERR_BAD_BASE    3   /* a byte outside {A,C,G,T,N}: see fqd_bad_base()     */
#define FQD_ERR_CAPACITY    4   /* more than 2^32-2 records in one engine             */
#define FQD_ERR_NO_DEVICE   5   /* no usable MI355X / HIP device                      */

/* where the caller's buffers live */
#define FQD_MEM_HOST        0
#define FQD_MEM_DEVICE      1

/* fqd_config.flags */
#define FQD_FLAG_PROFILE    1u  /* bracket every kernel with HIP events (fqd_profile) */
#define FQD_FLAG_NO_STAGE   2u  /* testing: force the per-lane global-load encoder    */
#define FQD_FLAG_WEAK_HASH  4u  /* testing: zero every hash's tag and its low 6 position bits,
                                   so unequal keys keep meeting in the table and the
                                   verify-then-probe-on branch runs on every insert.
                                   The flag alone does not make NEAR-EQUAL keys meet: the
                                   input has to hold them (tests/test_gpu_key_compare.py) */

typedef struct fqd_engine fqd_engine;

/* Replaces: HashDupRemover<T>::HashDupRemover(memlimit, tempdir, verbose)
 * (hash_dup_remover.hpp:77-78) + the `hashed_set records; records.reserve(ONE_MIL)`
 * of each driver (hpp:113-114,206-207,269-270). */
typedef struct fqd_config {
    int32_t  device;          /* HIP device ordinal                                       */
    int32_t  segments;        /* 1: setRecord keys (SE); 2: setRecordPair keys (PE)       */
    uint64_t capacity_reads;  /* hint: records expected over the engine's life (0 = grow) */
    uint64_t capacity_bases;  /* hint: total bases expected (0 = grow)                    */
    void*    stream;          /* hipStream_t to run on; NULL = the engine creates one     */
    uint32_t flags;           /* FQD_FLAG_*                                               */
    uint32_t reserved;
} fqd_config;

/* One mate's sequences for a batch: ASCII, one byte per base, no newlines
 * needed between reads.  Either ragged (offsets + lengths arrays, in the same
 * memory space as `bases`) or uniform (offsets == lengths == NULL: read i is
 * the uniform_len bytes at bases + i * uniform_stride).
 * Replaces the (obj.seq(), obj.seq_len()-1) pairs handed to the key
 * constructors at hash_dup_remover.hpp:124,131,223-224,234-235,293-294. */
typedef struct fqd_reads {
    const uint8_t*  bases;
    const uint64_t* offsets;
    const uint32_t* lengths;
    uint32_t        uniform_len;
    uint32_t        uniform_stride;
} fqd_reads;

typedef struct fqd_stats {
    uint64_t records;         /* records submitted so far (tot_reads, hpp:116)         */
    uint64_t duplicates;      /* keep flags cleared so far (dup_reads, hpp:116)        */
    uint64_t table_slots;     /* current capacity of the hash set                      */
    uint64_t key_bytes;       /* bytes of packed keys resident in HBM                  */
} fqd_stats;

/* Average device time per launch, measured with HIP events on the engine's
 * stream when FQD_FLAG_PROFILE is set (bench.py's roofline uses these). */
typedef struct fqd_profile {
    double   encode_ms;    uint64_t encode_launches;    uint64_t encode_reads;     /* encode_*_kernel            */
    double   insert_ms;    uint64_t insert_launches;    uint64_t insert_reads;     /* insert_kernel (atomic path) */
    double   partition_ms; uint64_t partition_launches; uint64_t partition_reads;  /* bulk path: hist + scatter passes, timed as one group per batch */
    double   dedup_ms;     uint64_t dedup_launches;     uint64_t dedup_reads;      /* bulk path: bucket_dedup_kernel */
    double   other_ms;     uint64_t other_launches;                                /* clears, scans, rehash      */
} fqd_profile;

int  fqd_abi_version(void);
int  fqd_device_count(int* count);

int  fqd_engine_create(const fqd_config* cfg, fqd_engine** out);
int  fqd_engine_destroy(fqd_engine* e);
/* Empties the set and the key store, keeping the allocations. */
int  fqd_engine_reset(fqd_engine* e);

/* Replaces one pass of the hot loop (hpp:126-144 SE, 228-248 PE) over `n`
 * records: builds their keys, probes/inserts them, and writes keep[i] = 1 if
 * record i (input order continues across calls) is the first with its key,
 * else 0.  `seg` points at cfg.segments descriptors.  `memory` says where
 * bases/offsets/lengths/keep live.  Device-space calls are asynchronous on
 * the engine's stream (the buffers must be complete on it: see the ORDERING RULE
 * at fqd_engine_wait_stream) and keep must stay valid until fqd_engine_sync();
 * host-space calls return with keep filled.  Flags of a batch are final when
 * it completes: later batches cannot change them. */
int  fqd_submit(fqd_engine* e, const fqd_reads* seg, uint64_t n, int memory, uint8_t* keep);

/* fqd_submit for the LAST batch of a run: the caller declares that nothing will be added before the next
 * fqd_engine_reset.  The reference's loop produces flags, not a set anyone looks at afterwards
 * (hash_dup_remover.hpp:126-144): the bulk insert path then leaves the set's segments where they were built
 * (on chip) instead of writing them back to HBM — 8 bytes per slot, 2 GiB for the 100 M-read table.  Same flags as
 * fqd_submit, bit for bit.  Afterwards fqd_submit* / fqd_insert_* fail with FQD_ERR_ARG until the engine is reset;
 * stats, flags and fqd_bad_base work as after fqd_submit. */
int  fqd_submit_final(fqd_engine* e, const fqd_reads* seg, uint64_t n, int memory, uint8_t* keep);

/* The hipStream_t the engine launches on (its own, or the one given in fqd_config), so a caller
 * can order its own work — copies, collectives — against the engine's with events. */
void* fqd_engine_stream(fqd_engine* e);

/* ORDERING RULE.  The engine runs on its own non-blocking stream (unless fqd_config.stream gave it the caller's) and
 * waits for nobody: a device buffer handed to any entry point of this header must be COMPLETE on the engine's stream
 * when the call is made — a fill, copy or kernel the caller queued on another stream (the null stream included) is
 * not ordered against the engine's work by itself and may land after it.  Two ways to order, besides a device-wide
 * synchronise: fqd_engine_wait_stream() before handing buffers over ("the engine starts after everything queued on
 * `stream` so far"), and fqd_stream_wait_engine() before the caller's stream reads what the engine wrote ("`stream`
 * continues after everything the engine has queued so far").  Both are an event record plus a stream wait: nothing
 * blocks on the host.  `stream` is a hipStream_t; NULL = the null stream. */
int  fqd_engine_wait_stream(fqd_engine* e, void* stream);
int  fqd_stream_wait_engine(fqd_engine* e, void* stream);

/* Waits for the stream and surfaces deferred errors (FQD_ERR_BAD_BASE). */
int  fqd_engine_sync(fqd_engine* e);

/* After FQD_ERR_BAD_BASE: the first offending byte in input order — record
 * index, segment (0/1), position in that sequence, and the byte itself — so a
 * caller can print the reference's two lines (seq_utils.cpp:18-19).  Keep flags
 * of records before `record` are valid. */
int  fqd_bad_base(const fqd_engine* e, uint64_t* record, uint32_t* segment, uint32_t* position, uint8_t* byte);

int  fqd_get_stats(fqd_engine* e, fqd_stats* out);
int  fqd_get_profile(fqd_engine* e, fqd_profile* out);
int  fqd_reset_profile(fqd_engine* e);
const char* fqd_last_error(const fqd_engine* e);   /* NULL engine: last create() failure */

/* ---- the two halves of fqd_submit, exposed for multi-GPU sharding ----------
 * (encode where the reads are, exchange fixed-size key records by
 * hash prefix with an all-to-all, insert at the owner.)  Uniform-length
 * batches only: every key of the engine has the same word count. */

/* Words (8 bytes each) of the packed key of a record with these mate lengths. */
uint32_t fqd_key_words(uint32_t len0, uint32_t len1);

/* Encodes n uniform reads into n*(key_words+1) uint64 at `records` (device):
 * record i = [hash, key words...].  Does not touch the set (any engine of the right `segments` serves). */
int  fqd_encode_uniform(fqd_engine* e, const fqd_reads* seg, uint64_t n, uint64_t* records);

/* The same for reads of SEVERAL lengths (trimmed reads; any descriptors, ragged or uniform): record i = [hash,
 * len0 | len1 << 32, key words..., zeros] with every key padded to the width of the longest read the caller allows
 * (max_len0, max_len1): fqd_padded_key_words(max_len0, max_len1) words after the hash.  Equal padded keys <=> equal
 * sequences of equal lengths, so such records travel through the fixed-size exchange like any others; their owner
 * holds them as opaque keys: fqd_reserve_keys / fqd_insert_keys / fqd_insert_slabs with len0 = fqd_padded_key_words(..)
 * and len1 = FQD_OPAQUE_KEYS.  A read longer than the maxima is an error (FQD_ERR_ARG at the next fqd_engine_sync). */
#define FQD_OPAQUE_KEYS 0xFFFFFFFFu
uint32_t fqd_padded_key_words(uint32_t max_len0, uint32_t max_len1);
int  fqd_encode_padded(fqd_engine* e, const fqd_reads* seg, uint64_t n, uint32_t max_len0, uint32_t max_len1, uint64_t* records);

/* Stable partition of n records by owner = (hash >> 40) % n_parts: `out_keys` gets the KEY WORDS of the records
 * grouped by owner in input order (the hash is left out: 8 bytes less per record on the wire; the owner recomputes
 * it), `counts` (device, n_parts uint64) the group sizes, `origin` (device, n uint32) the input position of each
 * output key.  fqd_reserve_keys: *slot (device) is room for n keys at the tail of the engine's key store — let the
 * exchange write the keys there, then pass *slot to fqd_insert_keys, which inserts them where they lie, in order
 * (first-occurrence-wins follows the order of arrival); no other engine call may come in between.  The owner is an
 * ordinary uniform engine whose keys lie back to back, aligned like everywhere else. */
int  fqd_partition_keys(fqd_engine* e, const uint64_t* records, uint64_t n, uint32_t key_words,
                        uint32_t n_parts, uint64_t* out_keys, uint64_t* counts, uint32_t* origin);
int  fqd_reserve_keys(fqd_engine* e, uint64_t n, uint32_t len0, uint32_t len1, uint64_t** slot);
int  fqd_insert_keys(fqd_engine* e, const uint64_t* keys, uint64_t n, uint32_t len0, uint32_t len1, uint8_t* keep);

/* An owner whose key shape has to change in mid-run: the reference keys a read of any length at any point of the
 * file (seq_utils.cpp:35-49, hash_dup_remover.hpp:126-144), while the exchange moves keys of ONE width.  Every key the
 * engine holds (from fqd_insert_keys / fqd_insert_slabs, with known mate lengths or opaque) is laid out again as an
 * opaque key of new_words words — [len0 | len1 << 32][key words][zeros], the form fqd_encode_padded gives the same
 * read under maxima with fqd_padded_key_words(..) == new_words — record numbers unchanged, the set rebuilt from the
 * new keys.  Afterwards the engine takes keys with len0 = new_words, len1 = FQD_OPAQUE_KEYS.  Waits for the stream. */
int  fqd_widen_keys(fqd_engine* e, uint32_t new_words);

/* The exchange with messages of FIXED size, so that an all-to-all can be queued before anybody knows how many keys
 * go where (fqd_shard below).  fqd_partition_slabs is fqd_partition_keys with part p's keys written to slab p — the
 * slab_cap key slots from out_keys + p * slab_cap * key_words — and the keys a slab has no room for written, part
 * after part, behind the last slab (from slot n_parts * slab_cap; counts[p] is the true count, so counts[p] - slab_cap
 * of them spilled).  origin (n_parts * slab_cap + n entries) = input position per slot, 0xFFFFFFFF for a slab slot
 * nothing went to — fqd_scatter_flags passes over those.  fqd_insert_slabs inserts n_slabs slabs of slab_cap slots
 * lying back to back at the slot fqd_reserve_keys(n_slabs * slab_cap) gave, of which slab j holds
 * min(slab_count[j], slab_cap) keys (slab_count on the device); the unused slots become records that nothing is ever
 * compared with, so the owner's record numbering — and with it first-occurrence-wins — follows (slab, position).
 * keep has n_slabs * slab_cap entries; those of unused slots mean nothing. */
int  fqd_partition_slabs(fqd_engine* e, const uint64_t* records, uint64_t n, uint32_t key_words, uint32_t n_parts,
                         uint64_t slab_cap, uint64_t* out_keys, uint64_t* counts, uint32_t* origin);
/* Encode + group in one call, with every owner's slab CUT into n_chunks sub-slabs of sub_cap slots, one per chunk of
 * chunk_reads consecutive reads of the batch (n <= n_chunks * chunk_reads): chunk c's keys for part p go, in input order,
 * to the slots from (p * n_chunks + c) * sub_cap on.  Cutting the slab the way the input is cut is what lets the keys be
 * written ONCE, straight to their place, by an encoder whose workgroups need nothing from each other (csrc/fqd_kernels.hpp,
 * encode_chunks) — where that applies: reads of one fixed length per mate, at most 16 parts, chunk_reads a multiple of 256.
 * chunk_counts[p * n_chunks + c] and totals[p] (device; totals has n_parts + 1 words, the last says which way the slabs
 * were filled: 0 sub-slab by sub-slab, 1 from their first slot on) are the TRUE counts; a key whose sub-slab is full is not written:
 * call again with FQD_SLABS_EXACT for the three-step path (fqd_encode_uniform + fqd_partition_slabs through an internal
 * buffer), which fills each slab from its first slot on — the same thing seen as full, partial and empty sub-slabs — and
 * writes what n_chunks * sub_cap slots cannot take to the spill region (chunk_counts shows it as a count above sub_cap in
 * the last sub-slab).  origin[] as fqd_partition_slabs has it.  Owner side: fqd_insert_slabs with n_parts_of_the_group *
 * n_chunks slabs of sub_cap slots. */
#define FQD_SLABS_EXACT 1u
int  fqd_encode_slabs(fqd_engine* e, const fqd_reads* seg, uint64_t n, uint32_t n_parts, uint64_t chunk_reads, uint32_t n_chunks,
                      uint64_t sub_cap, uint64_t* out_keys, uint64_t* chunk_counts, uint64_t* totals, uint32_t* origin, uint32_t flags);
int  fqd_insert_slabs(fqd_engine* e, const uint64_t* keys, uint32_t n_slabs, uint64_t slab_cap, const uint64_t* slab_count,
                      uint32_t len0, uint32_t len1, uint8_t* keep);
/* The same two with every key's 8-byte placement hash beside it, so that the owner does not have to read all 64 bytes
 * of every arrived key once more just to hash it (1.75 ms per 100 M reads of a 14 ms sharded step, measured on one rank;
 * it costs the links 12.5 % more bytes): fqd_encode_slabs_hashed also writes hash[slot] for every key slot it fills
 * (one-pass grouping only: after FQD_SLABS_EXACT, or whenever totals[n_parts] reads 1, out_hashes holds nothing and the
 * owner uses fqd_insert_slabs); fqd_insert_slabs_hashed takes the hashes as they arrived (device, n_slabs * slab_cap
 * words, overwritten where a slot holds no key) — keys of known mate lengths only: an owner of opaque (padded) keys
 * hashes the padded words, which the source never saw. */
int  fqd_encode_slabs_hashed(fqd_engine* e, const fqd_reads* seg, uint64_t n, uint32_t n_parts, uint64_t chunk_reads, uint32_t n_chunks,
                             uint64_t sub_cap, uint64_t* out_keys, uint64_t* out_hashes, uint64_t* chunk_counts, uint64_t* totals,
                             uint32_t* origin, uint32_t flags);
int  fqd_insert_slabs_hashed(fqd_engine* e, const uint64_t* keys, uint64_t* hashes, uint32_t n_slabs, uint64_t slab_cap,
                             const uint64_t* slab_count, uint32_t len0, uint32_t len1, uint8_t* keep);

/* ---- one dedup job over the GPUs of a node (BASELINE north_star: "reads are partitioned across the 8
 * GPUs of one node by hash prefix with an RCCL all-to-all over xGMI so each GPU owns a disjoint bucket range") ----
 * The reference runs on one core and has nothing to mirror here.  A shard group is `world` ranks with one engine
 * (one GPU) each; a process hosts n_local consecutive ranks of it — all of them (the CLI's FQD_DEVICES run, tests
 * with several ranks on one card) or one (bench.py: one process per GPU under torch.distributed.run).  Global input
 * order is (round, rank, position).  Per round every rank encodes its reads, writes the keys bound for owner
 * d = (hash >> 40) % world into slab d of its send buffer (fqd_partition_slabs), ONE all-to-all of fixed-size slabs
 * moves them — queued before any count has reached a host — and every owner inserts what it received in (source
 * rank, position) order (fqd_insert_slabs); the flags return through the reverse all-to-all.  Rounds are pipelined:
 * the flags of a round are on their way once the NEXT fqd_shard_round (or fqd_shard_flush) has returned.  A slab
 * that overflows (one owner drawing far more than its share) is settled by a second, exactly sized exchange before
 * the owner inserts anything of that round: results are exact whatever the skew. */
typedef struct fqd_shard fqd_shard;
#define FQD_SHARD_ID_BYTES 128
#define FQD_SHARD_RCCL 0    /* ncclSend/ncclRecv in one group per exchange: a direct all-to-all over xGMI */
#define FQD_SHARD_COPY 1    /* peer copies; every rank must live in this process (always used when ranks share a GPU) */
#define FQD_SHARD_PADDED 1u /* fqd_shard_config.flags: reads of several lengths, exchanged as padded keys (fqd_encode_padded) */
#define FQD_SHARD_SEND_HASH 2u /* fqd_shard_config.flags: every key's placement hash travels with it (72 instead of 64 bytes per
                                  150-base read on the links; the owners skip their re-hash pass).  Ignored with FQD_SHARD_PADDED. */

typedef struct fqd_shard_config {
    int32_t  world;            /* ranks of the job                                                        */
    int32_t  n_local;          /* ranks this process hosts: engines[0 .. n_local)                          */
    int32_t  first_rank;       /* global rank of engines[0]                                                */
    int32_t  transport;        /* FQD_SHARD_RCCL / FQD_SHARD_COPY                                          */
    uint64_t round_reads;      /* most records (pairs) one rank brings to a round                          */
    uint32_t len0, len1;       /* the job's fixed read lengths (len1 = 0: single-end); with FQD_SHARD_PADDED the
                                  longest reads allowed: batches of any lengths up to them, ragged or uniform */
    uint32_t slack_permille;   /* slab capacity over a fair share, 0 = 30                                  */
    uint32_t flags;            /* FQD_SHARD_PADDED, FQD_SHARD_SEND_HASH                                    */
    uint64_t slab_records;     /* 0 = fqd_shard_slab_capacity(...); tests force overflows with a small one */
    const uint8_t* unique_id;  /* RCCL: FQD_SHARD_ID_BYTES from fqd_shard_unique_id, the same in every process */
} fqd_shard_config;

typedef struct fqd_shard_stats {
    uint64_t rounds, overflow_rounds;       /* rounds started; rounds in which a slab to or from this rank overflowed */
    uint64_t bytes_sent, bytes_received;    /* over the exchange, both directions, self included                      */
    uint64_t slab_records;                  /* key slots per slab                                                     */
    double   exchange_ms;                   /* device time of the forward all-to-alls (HIP events on its stream)      */
    int32_t  transport, ranks_in_comm;      /* what is in use; ncclCommCount of this rank's communicator              */
} fqd_shard_stats;

/* Rank 0 of a multi-process group makes the id; every process hands the same bytes to fqd_shard_create. */
int  fqd_shard_unique_id(uint8_t* id);
uint64_t fqd_shard_slab_capacity(uint64_t round_reads, int32_t world, uint32_t slack_permille);
int  fqd_shard_create(fqd_engine* const* engines, const fqd_shard_config* cfg, fqd_shard** out);
int  fqd_shard_destroy(fqd_shard* s);
/* One round.  seg: n_local * segments descriptors (uniform, device memory), n: reads per local rank (0 allowed: every
 * rank of the group must call once per round), keep: one device array per local rank.  Asynchronous. */
int  fqd_shard_round(fqd_shard* s, const fqd_reads* seg, const uint64_t* n, uint8_t* const* keep);
/* Completes every round in flight and waits; FQD_ERR_BAD_BASE when an engine met a byte outside {A,C,G,T,N}
 * (fqd_bad_base of that engine: `record` counts within the round that held it). */
int  fqd_shard_flush(fqd_shard* s);
/* Waits until keep[] of round `round` (0-based count of fqd_shard_round calls) is final.  FQD_ERR_BAD_BASE when a
 * local engine had met a byte outside {A,C,G,T,N} by the time it had encoded that round: fqd_shard_bad_base names
 * the first one in input order among this process's ranks (`record` counts within the rank's batch of the round;
 * flags of the records before it are valid). */
int  fqd_shard_wait(fqd_shard* s, uint64_t round);
int  fqd_shard_bad_base(fqd_shard* s, uint64_t round, int32_t* local_rank, uint64_t* record, uint32_t* segment,
                        uint32_t* position, uint8_t* byte);
int  fqd_shard_get_stats(fqd_shard* s, int32_t local_rank, fqd_shard_stats* out);
const char* fqd_shard_last_error(const fqd_shard* s);   /* NULL: last create() failure */

/* ---- the `--unordered` read-ID join (hash_dup_remover.hpp:150-192,257-347) ------------
 * The reference sorts both files by ID tag on disk (ExternalSorter<T>::sort,
 * external_sort.hpp:66-71,88-215, order = FastqViewWithId::cmp, fastqview.cpp:168-178) and
 * merge-joins the sorted files (hpp:279-340).  Here both files' tags are ordered together in
 * HBM by one hand-written radix sort over an order-preserving compact code of the tags, and the
 * matches are read off the sorted union (csrc/fqd_join.hip).  All pointers are device pointers. */

/* ID tags of one file: the tag bytes of record i are bytes[offsets[i] .. offsets[i]+lengths[i]) —
 * anywhere, e.g. inside the file's raw text as uploaded.  n < 2^31. */
typedef struct fqd_tags {
    const uint8_t*  bytes;
    const uint64_t* offsets;
    const uint32_t* lengths;
    uint64_t        n;
} fqd_tags;

/* FastqViewWithId::read_new / FastaViewWithId::read_new (fastqview.cpp:190-204,
 * fastaview.cpp:153-167) for n records whose ID lines lie in `text`: id_start[i] = offset of the
 * leading '@' / '>', id_len[i] = length of the ID line including its newline.  Writes the tag's
 * offset into `text` and its length: after the first '.' of the line if there is one, else after
 * the first byte; up to the first ' ', else through the end of the line including the newline. */
int  fqd_extract_tags(fqd_engine* e, const uint8_t* text, const uint64_t* id_start, const uint32_t* id_len,
                      uint64_t n, uint64_t* tag_off, uint32_t* tag_len);

/* perm[k] (n uint32) = index of the record with the k-th smallest tag in the order of
 * FastqViewWithId::cmp: bytewise over the shorter length, shorter first on a tie; equal tags keep
 * their input order.  Replaces ExternalSorter<T>::sort. */
int  fqd_sort_tags(fqd_engine* e, const fqd_tags* t, uint32_t* perm);

/* Result arrays of fqd_join_tags (device memory provided by the caller). */
typedef struct fqd_join {
    uint32_t* perm_a;    /* a->n: record of file 1 with the i-th smallest tag                    */
    uint32_t* perm_b;    /* b->n: the same for file 2                                            */
    uint32_t* match_a;   /* a->n: sorted position in file 2 of the partner of sorted record i,
                            0xFFFFFFFF when it has none                                          */
    uint32_t* match_b;   /* b->n: sorted position in file 1 of the partner, or 0xFFFFFFFF        */
    uint32_t* pair_a;    /* min(a->n, b->n): record of file 1 of the k-th pair, in tag order     */
    uint32_t* pair_b;    /* min(a->n, b->n): record of file 2 of the k-th pair                   */
    uint64_t* n_pairs;   /* HOST: number of pairs                                                */
} fqd_join;

/* The merge-join of two tag-sorted files (hpp:283-309) without the sorted files: record x of
 * file 1 and record y of file 2 are a pair iff their tags are equal and they have the same rank
 * among the records with that tag in their files (k-th with k-th, which is what the merge loop
 * does to repeated IDs).  This is the FULL inner join; the reference's end-of-file rule
 * (hpp:281,317-340) only ever drops the last pair and is applied by the caller from
 * perm/match.  Returns after the stream has drained (n_pairs is known). */
int  fqd_join_tags(fqd_engine* e, const fqd_tags* a, const fqd_tags* b, const fqd_join* out);

/* off_out[k] = off_table[idx[k]], len_out[k] = len_table[idx[k]] for k < n: turns a pair list into
 * the ragged sequence descriptors (fqd_reads.offsets / lengths) of a dedup batch in tag order. */
int  fqd_gather_seqs(fqd_engine* e, const uint32_t* idx, uint64_t n, const uint64_t* off_table,
                     const uint32_t* len_table, uint64_t* off_out, uint32_t* len_out);

/* ---- device halves of the bounded-memory `--unordered` run (host streams both files twice) ------
 * dst[dst_off[i] .. +len[i]) = src[src_off[i] .. +len[i]) for i < n: copies what the join and the
 * dedup need of every record (tag, sequence) out of an uploaded block into stores that stay in HBM. */
int  fqd_copy_spans(fqd_engine* e, const uint8_t* src, const uint64_t* src_off, const uint32_t* len, uint64_t n,
                    uint8_t* dst, const uint64_t* dst_off);

/* *count (host) = number of records of t whose tag is <= the tag of record other_index of `other`, in
 * the order of FastqViewWithId::cmp (fastqview.cpp:168-178): where the merge-join's other cursor
 * stands when a record without a partner is consumed (the end-of-file rule needs it, hpp:281,317-340). */
int  fqd_count_tags_le(fqd_engine* e, const fqd_tags* t, const fqd_tags* other, uint64_t other_index, uint64_t* count);

/* ---- `--unordered` over several GPUs: every GPU joins one contiguous RANGE of the tag order ------------------------
 * The reference's two sorted files are one global order (external_sort.hpp, FastqViewWithId::cmp); here it is cut at
 * n_split splitters (tags picked from a sample: fqd_sample_tags writes the tag of every (n / n_samples)-th record, cut
 * to `stride` bytes, into out_bytes + k * stride / out_len[k]; the host sorts them and picks).  fqd_classify_tags:
 * range_out[i] = number of splitters that are < tag i (splitter j = split_bytes + j * split_stride, split_len[j] bytes,
 * ascending) — records with equal tags always land in the same range.  fqd_range_keep: keep[i] = (range[i] == which),
 * *count (host) = how many: with fqd_output_plan (idx = NULL) and fqd_copy_spans that moves a range's whole records,
 * in input order, into one contiguous piece of text for the GPU that owns the range.  fqd_max_u32: the largest of n
 * values (the longest sequence: the key width of the pair exchange).  All device pointers unless said otherwise. */
int  fqd_sample_tags(fqd_engine* e, const fqd_tags* t, uint32_t n_samples, uint32_t stride, uint8_t* out_bytes, uint32_t* out_len);
int  fqd_classify_tags(fqd_engine* e, const fqd_tags* t, const uint8_t* split_bytes, uint32_t split_stride, const uint32_t* split_len,
                       uint32_t n_split, uint32_t* range_out);
int  fqd_range_keep(fqd_engine* e, const uint32_t* range, uint64_t n, uint32_t which, uint8_t* keep, uint64_t* count);
int  fqd_max_u32(fqd_engine* e, const uint32_t* values, uint64_t n, uint32_t* max_out);

/* Where the survivors go: pair k (tag order, k < n) is written iff keep[k]; dest[idx[k]] = sum of
 * sizes[idx[j]] over the kept pairs j < k (byte offset of record idx[k] in this file's output), entries
 * of records that are not written keep what the caller preset; *total (host) = output size in bytes.
 * Replaces the sorted temporary files of the reference as the way records reach their place
 * (external_sort.hpp:107-112,209-215). */
int  fqd_output_offsets(fqd_engine* e, const uint8_t* keep, const uint32_t* idx, uint64_t n, const uint32_t* sizes,
                        uint64_t* dest, uint64_t* total);

/* The same for a run whose text stays in HBM, per PAIR instead of per record: for pair k (tag order, k < n)
 * src_off[k] = starts[idx[k]] (where record idx[k] lies in the text), len[k] = sizes[idx[k]] if keep[k] else 0,
 * dst_off[k] = sum of len[j], j < k (where it goes in the output); *total (host) = output size.  idx == NULL:
 * pair k is record k (an ordered run: the output keeps the input's order).  A window
 * [a, b) of pairs is then assembled in output order by one fqd_copy_spans over src_off+a, len+a, dst_off+a. */
int  fqd_output_plan(fqd_engine* e, const uint8_t* keep, const uint32_t* idx, uint64_t n, const uint64_t* starts,
                     const uint32_t* sizes, uint64_t* src_off, uint32_t* len, uint64_t* dst_off, uint64_t* total);

/* `.gz` output made in HBM: the n bytes at src (device; text of FASTQ/FASTA records, a record = `lines_per_record`
 * lines: 4 or 2) become BGZF — gzip members (RFC 1952) of at most 65280 input bytes, each carrying its
 * compressed size in a 'BC' extra field — written back to back at dst (device, dst_capacity >=
 * fqd_bgzf_bound(n)); *out_bytes (host) = their total size.  The end-of-file marker member is the caller's to
 * append.  One deflate block per member: literals, byte runs and matches against the same column one record up,
 * under one pair of dynamic Huffman codes per call; a member that would not shrink is stored; CRC-32 computed on
 * the device.  Any inflater reads it; the ratio is about that of zlib level 1-2.  Returns when dst is complete.
 * Replaces the gzip compressor the reference pushes onto its output stream (file_utils.hpp:71-82) for outputs
 * whose bytes are already on the device. */
uint64_t fqd_bgzf_bound(uint64_t n);
int  fqd_bgzf_deflate(fqd_engine* e, const uint8_t* src, uint64_t n, uint32_t lines_per_record,
                      uint8_t* dst, uint64_t dst_capacity, uint64_t* out_bytes);

/* The same with a choice of effort (added within ABI version 5: purely additive, nothing else changed).
 *   FQD_BGZF_FAST    what fqd_bgzf_deflate writes, byte for byte (it forwards here).
 *   FQD_BGZF_SEARCH  a real LZ77 search: a hash table of every member in LDS, 16 candidates a position anywhere
 *                    earlier in the member (distance <= 32768), the two structural candidates of the fast mode beside
 *                    them, one position of lazy look-ahead, a match taken only where the codes make it cheaper than its
 *                    literals.  Same framing, same bound, same stored fallback; 3-6 % smaller than zlib level 3 on
 *                    FASTQ text and 1-3 % above level 6 (member by member), at 3-4 GB/s instead of the fast mode's 140.
 * Any other effort: FQD_ERR_ARG.  Both modes are deterministic: equal input, equal bytes. */
#define FQD_BGZF_FAST   0u
#define FQD_BGZF_SEARCH 1u
int  fqd_bgzf_deflate_ex(fqd_engine* e, const uint8_t* src, uint64_t n, uint32_t lines_per_record, uint32_t effort,
                         uint8_t* dst, uint64_t dst_capacity, uint64_t* out_bytes);

/* BGZF input inflated in HBM: member m (m < n_members; all arrays device) is the raw deflate stream of comp_len[m]
 * bytes at comp + comp_off[m] and inflates to exactly out_len[m] (<= 65536) bytes at text + out_off[m] whose CRC-32
 * is crc[m] — what the host read off the member's header and trailer.  One wave per member.  *n_bad (host) =
 * members whose stream is damaged, ends early or late, or whose CRC differs; text is then to be discarded.
 * Replaces the gzip decompressor the reference pushes onto its input stream (file_utils.hpp:58-69). */
int  fqd_bgzf_inflate(fqd_engine* e, const uint8_t* comp, const uint64_t* comp_off, const uint32_t* comp_len,
                      const uint64_t* out_off, const uint32_t* out_len, const uint32_t* crc, uint64_t n_members,
                      uint8_t* text, uint64_t* n_bad);
/* An ORDINARY gzip file (members that are one long deflate stream without member sizes: what gzip, pigz and sequencer software
 * write; the reference reads it through the same gzip decompressor, file_utils.cpp:59-66) inflated in HBM.  `deflate` (device;
 * any alignment; 32 readable bytes behind the last one) points at the FIRST member's raw deflate stream — the caller has walked
 * its 10-byte-plus header — and avail_bytes says how many bytes of the file lie from there on (trailers and further members
 * included).  The stream is cut into units whose block starts are GUESSED; every unit is decoded on its own — by the wave
 * decoder of the BGZF reader, into two texts behind two made-up 32 KiB windows, so that what comes out says for every byte whether it is a byte of
 * the stream or a copy of a place of the window before the unit — the chain of unit ends and starts is checked (a wrong guess:
 * the unit is decoded again from the true boundary), the windows are made unit after unit, and the places become text
 * (csrc/fqd_gunzip.hip).  Further members are walked where a final block ends; every member's CRC-32 and ISIZE are held against
 * its trailer.  *ok = 1: text[0 .. *text_bytes) is the text of all members, *deflate_bytes the offset (from `deflate`) at which
 * the LAST member's deflate stream ends (its 8-byte trailer is the end of the file's data), *crc32 that member's CRC-32.
 * *ok = 0: a guess that could not be repaired, damaged data, a CRC or length that is not the trailer's, bytes behind the last
 * member that are no member, a unit that outgrew its room, a text longer than text_cap, or more than 32 MiB of packed bytes in
 * which no dynamic block starts (stored or fixed blocks only: one wave's work) — nothing is reported beyond that: the
 * caller reads the file the host way, which produces the reference-visible diagnostic.  Waits for the stream. */
int  fqd_gunzip(fqd_engine* e, const uint8_t* deflate, uint64_t avail_bytes, uint8_t* text, uint64_t text_cap,
                uint64_t* text_bytes, uint64_t* deflate_bytes, uint32_t* crc32, int32_t* ok);
/* The same for a file that is STILL BEING COPIED to HBM by another thread of the caller: *arrived (host memory) says how many of
 * the avail_bytes bytes from `deflate` on are in HBM and complete — the caller raises it as its copies finish (after the copy
 * stream has been waited for), never lowers it, and ends at avail_bytes; ~0 means "the rest will not come" and ends the call
 * with *ok = 0.  Block starts are looked for and units decoded as their bytes arrive, so that most of the call runs under the
 * read of the file; the call returns when everything has arrived and been dealt with.  arrived = NULL: everything is there. */
int  fqd_gunzip_arriving(fqd_engine* e, const uint8_t* deflate, uint64_t avail_bytes, const volatile uint64_t* arrived,
                         uint8_t* text, uint64_t text_cap, uint64_t* text_bytes, uint64_t* deflate_bytes, uint32_t* crc32, int32_t* ok);

/* The same for one BATCH of members of a file that is still being read: queued on the engine's stream, nothing waited
 * for; bad members are ADDED to the two uint64 at bad_counters (device; zeroed by the caller, read when it likes), so
 * the inflate of what has arrived runs under the read of what has not. */
int  fqd_bgzf_inflate_async(fqd_engine* e, const uint8_t* comp, const uint64_t* comp_off, const uint32_t* comp_len,
                            const uint64_t* out_off, const uint32_t* out_len, const uint32_t* crc, uint64_t n_members,
                            uint8_t* text, uint64_t* bad_counters);

/* The n bytes of text (device) cut into records the way the reference's views do it (fastqview.cpp:92-138,
 * fastaview.cpp:78-100): a record is lines_per_record lines (4: FASTQ, 2: FASTA), starts with '@' / '>', and a FASTQ
 * record's sequence and quality lines are equally long.  fqd_count_lines gives the number of newlines; the caller
 * sizes the arrays for n_records = lines / lines_per_record and fqd_scan_records fills, per record, start (offset of
 * its first byte), seq_off (of its sequence line), id_len (ID line with its newline), seq_len (without), size (whole
 * record).  *well_formed (host) = 1 iff the text is exactly n_records such records, ending with its last byte;
 * otherwise the arrays are not to be used and the caller reads the file the host way, which reproduces the
 * reference's diagnostics for whatever is wrong. */
int  fqd_count_lines(fqd_engine* e, const uint8_t* text, uint64_t n, uint64_t* n_lines);
int  fqd_scan_records(fqd_engine* e, const uint8_t* text, uint64_t n, uint32_t lines_per_record, uint64_t n_records,
                      uint64_t* start, uint64_t* seq_off, uint32_t* id_len, uint32_t* seq_len, uint32_t* size, int* well_formed);

/* ---- the sequence-based modes (`--compare-seq`; seq_dup_remover.hpp:40-218) ---------------------------------------
 * The reference sorts every record (pair) by sequence on disk (ExternalSorter<T> / PairedExternalSorter<T>,
 * paired_external_sort.hpp:20-33,128-135) and walks the sorted file with one comparator (comparator.cpp:45-91).  Here
 * both happen where the records lie in HBM (csrc/fqd_seq.hip, rules in csrc/fqd_seq_core.hpp).  A record's sequence is
 * given as an fqd_tags entry WITHOUT its '\n'; for pairs mate2 has mate1's n (NULL: single-end).  Device pointers. */
#define FQD_SEQ_TIGHT       0
#define FQD_SEQ_LOOSE       1
#define FQD_SEQ_HAMMING     2   /* `tail-hamming` */

/* perm[k] (n uint32) = index of the record (pair) with the k-th smallest sequence in the order of FastqView::cmp
 * (fastqview.cpp:56-67: bytewise over the shorter length with the '\n' counted, shorter first on a tie; pairs by mate 1,
 * then mate 2 — RecordPair::operator<).  Equal sequences keep their input order (the reference's order among them is an
 * artefact of std::sort and its chunking).  Any length; n < 2^31.  A sequence byte below '\n' (NUL, control bytes) is
 * refused with FQD_ERR_ARG: it would make strncmp and byte order disagree.  Returns after the stream has drained. */
int  fqd_sort_seqs(fqd_engine* e, const fqd_tags* mate1, const fqd_tags* mate2, uint32_t* perm);

/* head[k] (n bytes) = 1 iff the k-th record of perm is written by the reference's scan over the sorted records
 * (seq_dup_remover.hpp:54-109,131-218) with comparator `mode` (FQD_SEQ_*; `distance` for FQD_SEQ_HAMMING, ignored
 * otherwise); 0 = a duplicate of the last head before it.  *n_heads (host, may be NULL) = number of heads.  perm must
 * be an order of fqd_sort_seqs (loose mode relies on it).  Returns after the stream has drained. */
int  fqd_seq_heads(fqd_engine* e, const fqd_tags* mate1, const fqd_tags* mate2, const uint32_t* perm, int mode, uint32_t distance,
                   uint8_t* head, uint64_t* n_heads);

/* ---- `--compare-seq` on inputs larger than HBM: the sort order cut into ranges (added within ABI version 5: purely
 * additive).  The text goes through HBM one range of the sort order at a time; a range is chosen by the PREFIX KEY of
 * mate 1: its first 8 sequence bytes as a big-endian uint64, a sequence shorter than 8 padded with '\n'.  No accepted
 * byte is below '\n', so the key is monotone (non-strict) in the order of fqd_sort_seqs and equal sequences have equal
 * keys (rules and proofs: csrc/fqd_seq_range_core.hpp).
 *
 * fqd_seq_prefix_keys: for the n records of an uploaded block (mate1; the spans fqd_sort_seqs takes) key[i] (device, may
 * be NULL: check only).  Every sequence byte of the block is looked at, mate2's (may be NULL) as well: info->first_with[c]
 * (c < '\n') = the first record of the block that holds byte c in either mate, or ~0; info->bad_byte = the lowest such c,
 * or -1 — what the census of fqd_sort_seqs refuses, in its order.  info->longest[m] = the longest sequence of mate m.
 * size1 / size2 (device, may be NULL) are the records' sizes: bytes[i] (device, may be NULL) = size1[i] + size2[i]
 * (saturated at 2^32-1), added to what bytes[i] holds when `accumulate` is set (the mates of a pair arrive in blocks of
 * their own); info->record_bytes = their sum over the block.  Returns after the stream has drained. */
typedef struct fqd_seq_block_info {
    uint32_t longest[2];
    int32_t  bad_byte;
    uint32_t reserved;
    uint64_t record_bytes;
    uint64_t first_with[10];
} fqd_seq_block_info;
int  fqd_seq_prefix_keys(fqd_engine* e, const fqd_tags* mate1, const fqd_tags* mate2, const uint32_t* size1, const uint32_t* size2,
                         int accumulate, uint64_t* key, uint32_t* bytes, fqd_seq_block_info* info);

/* fqd_seq_plan_ranges: the EXACT plan from every pair's key and bytes (device, n < 2^32 pairs; every position is 64 bits
 * wide).  Ranges are cut only where the key changes; each is the longest run of whole key values whose bytes stay within
 * target_bytes; one key value that alone exceeds it is a range of its own.  range_of[i] (device, n uint32) = the range of
 * pair i, in input order.  table (HOST, max_ranges rows) = the ranges in key order; *n_ranges (host) = how many there are —
 * when that is more than max_ranges only the first max_ranges rows were written and range_of is not to be used: call again
 * with a larger table.  bytes_mate1 (device, may be NULL) = the part of bytes[i] that is mate 1's record: a row's
 * bytes_mate1 is its sum over the range (what the first file's store has to hold; the second's is bytes - bytes_mate1).
 * A plan of more than FQD_SEQ_MAX_RANGES ranges is refused with FQD_ERR_ARG as soon as the walk gets there (the inputs
 * are read once per range: such a target is a mistake, and the walk from cut to cut is one lane's work).  A copy of
 * (key, bytes) is sorted by the radix passes of the tag sort, the bytes are scanned in 64 bits, the cuts are found by
 * binary search from cut to cut; 24 bytes of scratch per pair during the call. */
#define FQD_SEQ_MAX_RANGES 65536u
typedef struct fqd_seq_range {
    uint64_t key_lo, key_hi;    /* the smallest and the largest key of the range */
    uint64_t pairs, bytes;
    uint64_t bytes_mate1;
} fqd_seq_range;
int  fqd_seq_plan_ranges(fqd_engine* e, const uint64_t* key, const uint32_t* bytes, const uint32_t* bytes_mate1, uint64_t n,
                         uint64_t target_bytes, uint32_t* range_of, fqd_seq_range* table, uint32_t max_ranges, uint32_t* n_ranges);

/* ---- FQD_SEQ_KEEP=best: the member of a cluster that is written (added within ABI version 5: purely additive).  Which
 * records form a cluster stays what fqd_seq_heads found; these two calls only choose the member that stands at the
 * head's place in the order, and so the record that the output plan and the writers take (rules and proofs:
 * csrc/fqd_seq_pick_core.hpp).
 *
 * fqd_seq_scores: score[i] (device, n uint32, input order) = the score of record (pair) i.  rec1 / rec2 (NULL: single-end)
 * give the WHOLE records as spans: offset = the record's first byte, length = its size with the final '\n'.  A record's
 * score is the sum of (b - 33) over the bytes b >= 33 of its last line without the '\n' (the quality line, Phred+33;
 * bytes below 33, a '\r' among them, count 0; an empty line scores 0), saturating at 2^32-1; a pair's is the saturating
 * sum of its mates'.  Reads every quality byte once.  Returns after the stream has drained.
 *
 * fqd_seq_pick_best: perm and head (device) are those of fqd_sort_seqs / fqd_seq_heads over n < 2^31 records; a cluster
 * is a run of places that starts at a set head flag (place 0 starts one whatever its flag says).  Per cluster the member
 * with the highest score, on equal scores the one earliest in the order, is the representative: perm[head place] and
 * perm[representative's place] are swapped.  The head flags do not move and no other entry of perm changes, so a cluster
 * of equal scores keeps its order.  *n_moved (host, may be NULL) = the clusters whose entry at the head's place changed.
 * 4 bytes of scratch per record during the call.  Returns after the stream has drained. */
int  fqd_seq_scores(fqd_engine* e, const fqd_tags* rec1, const fqd_tags* rec2, uint32_t* score);
int  fqd_seq_pick_best(fqd_engine* e, const uint32_t* score, const uint8_t* head, uint64_t n, uint32_t* perm, uint64_t* n_moved);

/* ---- FQD_FAST_KEEP / FQD_FAST_CLUSTERS: which record a `--fast` duplicate repeats (added within ABI version 5: purely
 * additive; fqd_submit and fqd_submit_final launch the same kernels with the same arguments as before).  Rules and
 * proofs: csrc/fqd_owner_core.hpp.
 *
 * fqd_submit_linked: fqd_submit (last == 0) or fqd_submit_final (last != 0) for FQD_MEM_DEVICE input, plus link (device,
 * n uint32): for every record of the batch whose flag is cleared, link[i] = the ENGINE index of an earlier record with
 * the identical key.  Entries of kept records are not written.  Which earlier record a link names depends on how the
 * batch was scheduled; callers rely on "earlier, same key" only.  Any other memory space is FQD_ERR_ARG.
 *
 * fqd_owners: keep and link (device) are those of ALL n records submitted so far (every batch through
 * fqd_submit_linked, flags and links at the records' engine indices).  owner[i] (device, n uint32) = i where keep[i],
 * else the kept record the chain of links from i ends at: the first record with i's key.  Does not use the table (works
 * after the final batch).  Returns after the stream has drained; a link that does not decrease is FQD_ERR_ARG.
 *
 * fqd_group_owners: perm (device, n uint32) = the records ordered by owner, the members of an owner in input order;
 * head[k] (device, n bytes) = 1 at the first place of every run; *n_clusters (host, may be NULL) = the runs.  n < 2^31.
 * 24 bytes of scratch per record during the call.  Returns after the stream has drained.
 *
 * fqd_heads_to_keep: keep[perm[k]] = head[k] for k < n (all device): after fqd_seq_pick_best over (perm, head) the
 * record at every head's place is the one to write.  Returns after the stream has drained. */
int  fqd_submit_linked(fqd_engine* e, const fqd_reads* seg, uint64_t n, int memory, uint8_t* keep, uint32_t* link, int last);
int  fqd_owners(fqd_engine* e, const uint8_t* keep, const uint32_t* link, uint64_t n, uint32_t* owner);
int  fqd_group_owners(fqd_engine* e, const uint32_t* owner, uint64_t n, uint32_t* perm, uint8_t* head, uint64_t* n_clusters);
int  fqd_heads_to_keep(fqd_engine* e, const uint32_t* perm, const uint8_t* head, uint64_t n, uint8_t* keep);

/* ---- FQD_FAST_STRAND=both: the orientation a read (pair) is keyed in (added within ABI version 5: purely additive; no
 * existing entry launches anything new).  Rule and proofs: csrc/fqd_strand_core.hpp.  Single-end: the canonical form of a
 * read s is the bytewise smaller of s and its reverse complement (A<->T, C<->G, every other byte as it is); flipped = the
 * reverse complement is strictly smaller.  Pairs: the canonical form of (mate 1, mate 2) has the smaller mate first — bytewise
 * over the shorter length, the shorter first on a tie; nothing is complemented; flipped = mate 2 is strictly smaller.  Two
 * records are copies of one fragment, whichever strand each came from, exactly when their canonical forms are identical.
 *
 * fqd_canonical_reads: device memory only.  seg = the engine's `segments` descriptors, ragged or uniform as in fqd_submit.
 * The canonical sequences of the n records are packed back to back, in input order, into out: record i's first canonical
 * mate at out_off0[i] with out_len0[i] bytes, then (paired engines) its second at out_off1[i] = out_off0[i] + out_len0[i]
 * with out_len1[i] bytes; the offsets are exclusive prefix sums in 64 bits, the total is exactly the input's sequence bytes.
 * out_capacity below that total: FQD_ERR_ARG, and none of the output arrays is written.  flipped[i] (n bytes) = 1 where
 * record i was turned; *n_flipped (host, may be NULL) = how many.  {out, out_off0, out_len0} and {out, out_off1, out_len1}
 * are fqd_reads that fqd_submit* take.  out_off1 and out_len1 are NULL for a single-end engine (anything else: FQD_ERR_ARG).
 * Queued on the engine's stream and not waited for, except: with n_flipped the call returns after the stream has drained,
 * and with ragged descriptors it waits for its size scan (8 bytes come back) before it queues the rest. */
int  fqd_canonical_reads(fqd_engine* e, const fqd_reads* seg, uint64_t n, uint8_t* out, uint64_t out_capacity,
                         uint64_t* out_off0, uint32_t* out_len0, uint64_t* out_off1, uint32_t* out_len1,
                         uint8_t* flipped, uint64_t* n_flipped);

/* ---- FQD_FAST_UMI=colon|underscore: the unique molecular identifier in a record's ID line as part of its key (added
 * within ABI version 5: purely additive; no existing entry launches anything new).  Rule and proofs:
 * csrc/fqd_umi_core.hpp.  The first word W of an ID line is what stands behind its leading '@' / '>' up to the first of
 * ' ', '\t', '\r', '\n'; the UMI field U is what stands in W behind its LAST separator byte (sep: ':' or '_'); '+', '-'
 * and '_' inside U join the halves of a dual UMI, every other byte of U is one of A C G T N; U's shape is its length and
 * the set of its places that hold a joiner, and it is the same for every record of a run.  The key of a record is U's bases
 * in front of mate 1's sequence.
 *
 * fqd_umi_find: device memory only (info: host).  Line i is the id_len[i] bytes at text + id_start[i].  umi_off[i] (n
 * uint32) = U's offset inside line i: the last separator's position + 1, 0 where W holds none.  *info: umi_len, joiners
 * (bit p = U[p] is a joiner) and n_bases = umi_len - popcount(joiners) are record 0's shape (all 0 when record 0 is
 * refused or n = 0); bad_record = the LOWEST record that is refused (FQD_UMI_NO_RECORD: none) and bad_reason why — the
 * first of FQD_UMI_NO_SEPARATOR .. FQD_UMI_SHAPE_DIFFERS that holds for it, in that order.  Nothing else is written.
 * Returns after the stream has drained (once).
 *
 * fqd_umi_reads: device memory only (info: host, as fqd_umi_find left it with no record refused — anything else is
 * FQD_ERR_ARG).  mate0 = ONE descriptor, ragged or uniform as in fqd_submit: mate 1's sequences.  Record i's key bytes — the
 * n_bases bases of its U, then its sequence — are packed back to back, in input order, into out at out_off[i] with
 * out_len[i] = n_bases + its length; the offsets are exclusive prefix sums in 64 bits.  out_capacity below their total:
 * FQD_ERR_ARG, and none of the output arrays is written.  {out, out_off, out_len} is an fqd_reads that fqd_submit* take
 * for mate 1.  Queued on the engine's stream and not waited for, except that with ragged descriptors it waits for its size
 * scan (8 bytes come back) before it queues the rest. */
#define FQD_UMI_NO_RECORD 0xFFFFFFFFFFFFFFFFull
enum fqd_umi_reason {
    FQD_UMI_OK = 0,
    FQD_UMI_NO_SEPARATOR = 1,   /* W holds no separator */
    FQD_UMI_EMPTY = 2,          /* U is empty: the separator is W's last byte */
    FQD_UMI_TOO_LONG = 3,       /* U is longer than 64 bytes */
    FQD_UMI_BAD_BYTE = 4,       /* U holds a byte outside ACGTN+-_ */
    FQD_UMI_NO_BASE = 5,        /* U holds joiners only */
    FQD_UMI_SHAPE_DIFFERS = 6   /* U's length or joiner places differ from record 0's */
};
typedef struct fqd_umi_info {
    uint32_t n_bases;           /* Lb */
    uint32_t umi_len;
    uint64_t joiners;
    uint64_t bad_record;
    uint32_t bad_reason;        /* enum fqd_umi_reason */
    uint32_t reserved;
} fqd_umi_info;
int  fqd_umi_find(fqd_engine* e, const uint8_t* text, const uint64_t* id_start, const uint32_t* id_len, uint64_t n, int sep,
                  uint32_t* umi_off, fqd_umi_info* info);
int  fqd_umi_reads(fqd_engine* e, const uint8_t* text, const uint64_t* id_start, const uint32_t* umi_off, const fqd_umi_info* info,
                   const fqd_reads* mate0, uint64_t n, uint8_t* out, uint64_t out_capacity, uint64_t* out_off, uint32_t* out_len);

/* ---- FQD_FAST_SIZEOUT / FQD_FAST_LEVELS: every cluster's member count, as a `;size=N` label on the written record and as
 * a table of duplication levels (added within ABI version 5: purely additive; no existing entry launches anything new).
 * Rules and proofs: csrc/fqd_size_core.hpp.  (perm, head) is an order of the n records and a flag at the first place of
 * every cluster — fqd_group_owners', after fqd_seq_pick_best where a member was picked, so that the record at a head's
 * place is the written one; any other (perm, head) of that shape, fqd_sort_seqs / fqd_seq_heads' among them, serves as well.
 *
 * fqd_cluster_sizes: device memory only (levels: host, may be NULL).  A run is a head place and the places behind it up
 * to the next head; size[perm[k]] (n uint32) = the run's length where head[k], 0 at every other place: every entry of size
 * is written exactly once.  levels: row L counts the runs whose length falls in level L — 1 .. 9 one row each, then 10-49,
 * 50-99, 100-499, 500-999, 1000-4999, 5000-9999, 10000+ — and sums their lengths; largest = the longest run (all 0 for
 * n = 0).  n < 2^31.  head[0] == 0 with n > 0 is FQD_ERR_ARG and nothing is written to size.  A max-scan in three launches
 * (tile values, one block over them, the places), no block waiting for another; 4 bytes of scratch per 2048 records.
 * Returns after the stream has drained.
 *
 * fqd_size_labels: device memory only; all arrays per record r < n of ONE file (called once per file).  The ID line of
 * record r is the id_len[r] bytes at text + start[r], its '\n' included.  label_at[r] (n uint32) = the length of '@' / '>'
 * and the line's first word: the position of the first ' ', '\t', '\r' or '\n' behind position 0, id_len[r] where there is
 * none.  An ID line that already holds `;size=` is not looked at.  out_size[r] (n uint32) = rec_size[r] + 6 + the decimal
 * digits of size[r] where keep[r], rec_size[r] elsewhere: what fqd_output_plan takes for `sizes`, so that its len and dst_off
 * leave room for the labels.  A kept record whose size is 0 is FQD_ERR_ARG (counted on the device, reported once).  Returns
 * after the stream has drained.
 *
 * fqd_copy_labelled: fqd_copy_spans with a label, all arrays per span i < n (a window passes every array advanced by its
 * first span, as with fqd_copy_spans).  len[i] is the GROWN length that fqd_output_plan produced from out_size, 0 for a span
 * that is not written.  dst + dst_off[i] receives the first label_at[i] bytes at src + src_off[i], then `;size=<size[i]>`,
 * then the remaining len[i] - label_at[i] - label bytes of the source.  Only launches. */
typedef struct fqd_size_levels {
    uint64_t clusters[16];      /* runs per level */
    uint64_t records[16];       /* the sum of their lengths */
    uint32_t largest;
    uint32_t reserved;
} fqd_size_levels;
int  fqd_cluster_sizes(fqd_engine* e, const uint32_t* perm, const uint8_t* head, uint64_t n, uint32_t* size, fqd_size_levels* levels);
int  fqd_size_labels(fqd_engine* e, const uint8_t* text, const uint64_t* start, const uint32_t* id_len, const uint32_t* rec_size,
                     const uint8_t* keep, const uint32_t* size, uint64_t n, uint32_t* label_at, uint32_t* out_size);
int  fqd_copy_labelled(fqd_engine* e, const uint8_t* src, const uint64_t* src_off, const uint32_t* len, const uint32_t* label_at,
                       const uint32_t* size, uint64_t n, uint8_t* dst, const uint64_t* dst_off);

/* ---- FQD_FAST_SORT=size / FQD_FAST_MINSIZE / FQD_FAST_MAXSIZE: the written records in order of decreasing cluster size,
 * and clusters outside size bounds not written at all (added within ABI version 5: purely additive; no existing entry
 * launches anything new).  Rules and proofs: csrc/fqd_size_order_core.hpp.  (perm, head), size and keep are those of
 * fqd_cluster_sizes and fqd_size_labels above: size[r] = the member count at every written record r, 0 elsewhere, and
 * keep[r] set at the written records.
 *
 * fqd_size_filter: device memory only (the two counts: host, each may be NULL).  For every record r < n with keep[r] set
 * and size[r] < min_size, or max_size != 0 and size[r] > max_size: keep[r] is cleared, *clusters_dropped counts it and
 * *records_dropped adds size[r].  No other flag is written.  1 <= min_size <= 2^31-1; max_size = 0 (no upper bound) or
 * min_size <= max_size <= 2^31-1; n < 2^31; anything else is FQD_ERR_ARG and nothing is launched.  A kept record whose size
 * is 0 — flags and sizes that do not belong together — is FQD_ERR_ARG (counted on the device, reported once): nothing is
 * promised about keep then, and the counts stay 0.  One streaming pass, the counters summed wave by wave and block by block
 * (three atomics a block, none per record).  Returns after the stream has drained.
 *
 * fqd_size_order: device memory only (n_written: host, not NULL).  A kept place is a place s with head[s] set and
 * keep[perm[s]] set.  Take the kept places in ascending order and sort them STABLY by size[perm[s]] descending:
 * order[k] = perm[s] of the k-th, for k < W = *n_written, their number.  Among clusters of one size the one whose first
 * member stands earlier in the input comes first (the order of `<output>.clusters`).  Entries of order at W and beyond are
 * not touched; W = 0 leaves order as it is.  n < 2^31.  head[0] == 0 with n > 0 is FQD_ERR_ARG, and so is a kept place of size
 * 0: in both cases nothing is written to order.  An order that is no permutation of 0 .. n-1 never makes the call read
 * outside keep[0 .. n) and size[0 .. n) or write outside order[0 .. n): W <= the number of head places <= n.  The kept places
 * are compacted by an exclusive count in three launches (tile counts, one block over them, the places; no block waits for
 * another), then sorted in two tiers: ONE 8-bit pass over all W entries tells the sizes 1 .. 255 apart and collects the L
 * clusters above 255 members, and only those L <= n / 256 entries go through the passes that the largest size needs.
 * Scratch during the call: 8 bytes per 2048 records and 24 bytes per kept place, plus 1 KiB per 4096 kept places.  Two counts
 * come back in between (W; L and the largest size); returns after the stream has drained.
 *
 * fqd_size_order_ex: fqd_size_order, which also reports what the call itself counted and did (info: host, may be NULL;
 * all 0 where the call fails or writes nothing): written = W; large = L, the pairs tier 2 sorted apart; largest = the largest
 * size among the kept places; tier2_passes = the 8-bit passes launched over those L pairs (0 where L <= 1 or all of them
 * have one size).
 *
 * fqd_take_u32: out[k] = values[idx[k]] for k < n (all device; values holds an entry for every idx[k], which the caller
 * guarantees; out overlaps neither input): brings a per-record array into the written order.  Only launches. */
int  fqd_size_filter(fqd_engine* e, const uint32_t* size, uint64_t n, uint32_t min_size, uint32_t max_size, uint8_t* keep,
                     uint64_t* clusters_dropped, uint64_t* records_dropped);
int  fqd_size_order(fqd_engine* e, const uint32_t* perm, const uint8_t* head, const uint32_t* size, const uint8_t* keep, uint64_t n,
                    uint32_t* order, uint64_t* n_written);
typedef struct fqd_size_order_info {
    uint64_t written;
    uint64_t large;
    uint32_t largest;
    uint32_t tier2_passes;
} fqd_size_order_info;
int  fqd_size_order_ex(fqd_engine* e, const uint32_t* perm, const uint8_t* head, const uint32_t* size, const uint8_t* keep, uint64_t n,
                       uint32_t* order, uint64_t* n_written, fqd_size_order_info* info);
int  fqd_take_u32(fqd_engine* e, const uint32_t* values, const uint32_t* idx, uint64_t n, uint32_t* out);

/* ---- FQD_FAST_SIZEIN=1: a `;size=N` that the input's ID lines already carry is the record's weight, a cluster's size is the
 * sum of its members' weights, and the new label takes the old annotation's place (added within ABI version 5: purely
 * additive; no existing entry launches anything new).  Rules and proofs: csrc/fqd_sizein_core.hpp.  W is the first word of
 * an ID line as above.  A candidate is a position p >= 1 at which the six bytes `;size=` stand inside W, compared exactly; it
 * is well-formed when 1 .. 10 decimal digits follow (leading zeros allowed), then W's end or a ';', and the value is in
 * 1 .. 2^31-1.  No candidate: weight 1.  Exactly one, well-formed: weight = its value, and the annotation is the bytes
 * `;size=<digits>`.  Anything else refuses the record, for the first of these that holds of the FIRST candidate from the
 * left: FQD_SIZEIN_NO_DIGITS; FQD_SIZEIN_TOO_LARGE for eleven digits or more (no more are looked at); FQD_SIZEIN_BAD_END for
 * another byte behind the digits; FQD_SIZEIN_ZERO; FQD_SIZEIN_TOO_LARGE for a value above 2^31-1; FQD_SIZEIN_TWICE where a
 * second candidate follows.
 *
 * fqd_size_annotations: device memory only (info: host, not NULL), all arrays per record r < n of ONE file.  Line r is the
 * id_len[r] bytes at text + start[r].  weight, label_at and cut are n uint32 each and each may be NULL: weight[r] as above;
 * label_at[r] = the annotation's start, or the first word's end where there is none (fqd_size_labels' value); cut[r] = the
 * annotation's length, 0 for none.  expect (may be NULL: file 1) = file 1's weights for a call over file 2: an annotation in
 * line r must then say expect[r], FQD_SIZEIN_MATES_DIFFER otherwise; a line without one is fine.  *info: bad_record = the
 * LOWEST refused record (FQD_UMI_NO_RECORD: none) and bad_reason why; annotated = the records with an annotation and
 * total_weight = the sum of the weights (both of the records that are not refused).  A refused record makes the call return
 * FQD_OK with info set; the arrays' contents are then unspecified.  n <= 2^32-2.  Sixteen lanes a record, one launch; returns
 * after the stream has drained (once).
 *
 * fqd_cluster_weights: fqd_cluster_sizes with a weight per record (device memory only; levels: host, may be NULL; info: host,
 * not NULL).  size[perm[s]] (n uint32) = the sum of weight[perm[k]] over the run that starts at head place s, 0 at every
 * other place: every entry is written exactly once.  levels as in fqd_cluster_sizes, from the weighted sizes.  Sums are 64-bit
 * throughout.  A run whose sum exceeds 2^31-1 is reported: info->over_record = the lowest record at the head place of such a
 * run (FQD_UMI_NO_RECORD: none), over_sum = that run's exact sum; the call returns FQD_OK, levels is all 0 and nothing is
 * promised about size.  n < 2^31.  head[0] == 0 with n > 0 (nothing is written to size), or a weight of 0 (counted on the
 * device, reported once), is FQD_ERR_ARG.  One segmented sum in three launches (tile values, one block over them, the
 * places), no block waiting for another; 16 bytes of scratch per 2048 records.  Returns after the stream has drained.
 *
 * fqd_size_relabel: device memory only, elementwise: out_size[r] = rec_size[r] - cut[r] + 6 + the decimal digits of size[r]
 * where keep[r], rec_size[r] elsewhere — what fqd_output_plan takes for `sizes`.  A kept record whose size is 0 is FQD_ERR_ARG
 * (counted on the device, reported once).  Returns after the stream has drained.
 *
 * fqd_copy_relabelled: fqd_copy_labelled that leaves the cut[i] bytes behind label_at[i] out: dst + dst_off[i] receives the
 * first label_at[i] bytes at src + src_off[i], then `;size=<size[i]>`, then the source from label_at[i] + cut[i] on, len[i]
 * bytes in all (the GROWN length that fqd_output_plan produced from fqd_size_relabel's out_size, 0 for a span that is not
 * written).  cut[i] = 0 is fqd_copy_labelled.  Only launches. */
enum fqd_sizein_reason {
    FQD_SIZEIN_OK = 0,
    FQD_SIZEIN_NO_DIGITS = 1,    /* `;size=` and no digit behind it */
    FQD_SIZEIN_BAD_END = 2,      /* the digits are followed by something other than ';' or the word's end */
    FQD_SIZEIN_ZERO = 3,         /* the value is 0 */
    FQD_SIZEIN_TOO_LARGE = 4,    /* more than 10 digits, or a value above 2^31-1 */
    FQD_SIZEIN_TWICE = 5,        /* a well-formed annotation and another `;size=` behind it */
    FQD_SIZEIN_MATES_DIFFER = 6  /* file 2's annotation does not say file 1's weight */
};
typedef struct fqd_sizein_info {
    uint64_t bad_record;
    uint32_t bad_reason;        /* enum fqd_sizein_reason */
    uint32_t reserved;
    uint64_t annotated;
    uint64_t total_weight;
} fqd_sizein_info;
typedef struct fqd_weights_info {
    uint64_t over_record;
    uint64_t over_sum;
} fqd_weights_info;
int  fqd_size_annotations(fqd_engine* e, const uint8_t* text, const uint64_t* start, const uint32_t* id_len, uint64_t n, const uint32_t* expect,
                          uint32_t* weight, uint32_t* label_at, uint32_t* cut, fqd_sizein_info* info);
int  fqd_cluster_weights(fqd_engine* e, const uint32_t* perm, const uint8_t* head, const uint32_t* weight, uint64_t n, uint32_t* size,
                         fqd_size_levels* levels, fqd_weights_info* info);
int  fqd_size_relabel(fqd_engine* e, const uint32_t* rec_size, const uint8_t* keep, const uint32_t* size, const uint32_t* cut, uint64_t n,
                      uint32_t* out_size);
int  fqd_copy_relabelled(fqd_engine* e, const uint8_t* src, const uint64_t* src_off, const uint32_t* len, const uint32_t* label_at,
                         const uint32_t* cut, const uint32_t* size, uint64_t n, uint8_t* dst, const uint64_t* dst_off);

/* ---- FQD_FAST_UMI_MISMATCH=1|2: exact UMI clusters of one sequence that differ in a base or two are one molecule (added
 * within ABI version 5: purely additive; no existing entry launches anything new).  Rule and proofs:
 * csrc/fqd_umi_merge_core.hpp.  A sequence group is the records with identical sequences (UMI left out); a node is one
 * distinct B(U) in it — an exact cluster — with count = its members and first = its first record; dist = the places at which
 * two nodes' B(U) differ; a -> b where dist(a, b) <= distance and count(a) >= 2 count(b) - 1 (UMI-tools' directional rule);
 * root(v) = the node of highest count, on equal counts of lowest first record, among v and the nodes with a directed path
 * to v; the records of all nodes with one root are one merged cluster.
 *
 * fqd_umi_merge: device memory only (info, out: host).  text, id_start, umi_off and info are fqd_umi_find's over the same n
 * records (an info that names a refused record: FQD_ERR_ARG).  owner_exact = fqd_owners of the run keyed B(U) ‖ sequence,
 * owner_seq = fqd_owners of a second run over the same records keyed by the sequences alone, size = fqd_cluster_sizes over
 * the exact grouping (the count at every cluster's first record).  distance is 1 or 2 (anything else: FQD_ERR_ARG).
 * owner_out[i] (n uint32) = the first record, in input order, of record i's merged cluster; fqd_group_owners takes it.
 * owner_out must not overlap the inputs.  *out: nodes; groups = the sequence groups of more than one node; merged = the
 * nodes whose root is another node (the merged clusters number nodes - merged); largest = the nodes of the largest group;
 * sweeps = the most label sweeps that changed something in any group (the longest shortest path from a root to a node of
 * its cluster); max_group = FQD_UMI_MERGE_MAX_GROUP.  A group of more nodes than that is refused: over_limit_first = the
 * lowest first record of such a group (FQD_UMI_NO_RECORD: there is none), over_limit_nodes = that group's nodes; the call
 * returns FQD_OK, owner_out is NOT written, merged and sweeps are 0.  An owner behind its record, or size 0 at a record that
 * owns itself, is FQD_ERR_ARG (counted on the device, nothing written).  n < 2^31.  Scratch during the call: 4 bytes a record
 * and (34 + 8 * ceil(n_bases / 16)) bytes a node.  Two 64-bit results come back in between (the nodes, the groups per size
 * class); returns after the stream has drained.  stage_ms is a diagnostic (tools/umi_merge_probe.py): the wall time of the
 * three parts the call's own waits cut it into, launches and waits included. */
#define FQD_UMI_MERGE_MAX_GROUP 4096u
typedef struct fqd_umi_merge_info {
    uint64_t nodes;
    uint64_t groups;
    uint64_t merged;
    uint32_t largest;
    uint32_t sweeps;
    uint32_t max_group;
    uint32_t over_limit_nodes;
    uint64_t over_limit_first;
    float    stage_ms[4];       /* host wall time between the call's own synchronisations: nodes, group + classes, merge + spread; 0 */
} fqd_umi_merge_info;
int  fqd_umi_merge(fqd_engine* e, const uint8_t* text, const uint64_t* id_start, const uint32_t* umi_off, const fqd_umi_info* info,
                   const uint32_t* owner_exact, const uint32_t* owner_seq, const uint32_t* size, uint64_t n, uint32_t distance,
                   uint32_t* owner_out, fqd_umi_merge_info* out);

/* keep[i] = (owner[i] == i) for i < n (all device): the flags of a grouping given by its owners — what fqd_umi_merge leaves.
 * Only launches. */
int  fqd_owners_to_keep(fqd_engine* e, const uint32_t* owner, uint64_t n, uint8_t* keep);

/* ---- FQD_FAST_OPTICAL=D: only optical duplicates are duplicates — copies of a read that lie within D pixels of each other on
 * one tile of the flow cell (added within ABI version 5: purely additive; no existing entry launches anything new).  Rule and
 * proofs: csrc/fqd_optical_core.hpp.  W is the first word of an ID line as above, split at ':' into fields
 * (instrument:run:flowcell:lane:tile:x:y[:UMI]).  The surface of a record is the bytes of fields 1 .. 4 with the colons between
 * them; tile and x are fields 5 and 6, 1 .. 9 decimal digits each; y is the leading 1 .. 9 digits of field 7, followed by the
 * field's end or one of ':' '_' '#' '/'.  Two records are neighbours when their surfaces are bytewise identical, their tiles
 * equal and |xa - xb| <= D and |ya - yb| <= D; an optical group is a connected component of that relation among the records of
 * one cluster, owned by its first member in input order.
 *
 * fqd_read_places: device memory only (info: host, not NULL), all arrays per record r < n.  Line r is the id_len[r] bytes at
 * text + id_start[r].  tile, x, y (n uint32 each) as above; surface[r] (n uint32) = the surface's length in bytes, with
 * FQD_PLACE_SAME_SURFACE set where the surface is record 0's (almost every run has one surface, and the split compares the
 * bytes only of two records that both lack the bit).  *info: bad_record = the LOWEST record that is refused
 * (FQD_UMI_NO_RECORD: none) and bad_reason why — the first of FQD_PLACE_FEW_FIELDS, FQD_PLACE_EMPTY_FIELD, then of tile's, x's
 * and y's own reason in that order; other_surface = the records, of those not refused, whose surface is not record 0's.  A
 * refused record makes the call return FQD_OK with info set; the arrays' contents are then unspecified.  n <= 2^32-2.  Sixteen
 * lanes a record, one launch, no load outside an ID line; returns after the stream has drained (once).
 *
 * fqd_optical_split: device memory only (out: host, not NULL).  (perm, head) = fqd_group_owners' over the current owners: the
 * members of a cluster in input order; tile, x, y, surface = fqd_read_places' over the same n records, text and id_start its
 * inputs (the surface of record r is read at text + id_start[r] + 1).  distance = D, 1 .. 2^31-1.  owner_out[i] (n uint32) =
 * the first record, in input order, of record i's optical group; fqd_group_owners and fqd_owners_to_keep take it.  owner_out
 * must not overlap an input (FQD_ERR_ARG).  *out: clusters_in = the clusters of (perm, head); clusters_out = the optical
 * groups; split = the clusters that fell apart into more than one; largest = the members of the largest cluster; sweeps = the
 * most label sweeps any cluster took (a sweep = a min step that changed a label, and the pointer jump behind it);
 * max_cluster = FQD_OPTICAL_MAX_CLUSTER.  A cluster of more members than that is refused: over_limit_first = the lowest first
 * record of such a cluster (FQD_UMI_NO_RECORD: there is none), over_limit_members = that cluster's members; the call returns
 * FQD_OK, owner_out is NOT written, clusters_out, split and sweeps are 0.  head[0] == 0, or an order that names a record outside
 * 0 .. n-1, is FQD_ERR_ARG (counted on the device, nothing written).  n < 2^31.  Clusters go by size: one member — a store; up
 * to 8 — eight lanes; up to 64 — a wave; up to 2048 — a workgroup, places and labels in LDS; beyond — a thread a member over
 * many workgroups, two launches a sweep, the labels in scratch.  Scratch during the call: 4 bytes a cluster, about 5 bytes a
 * record for the lists and, for inputs of more than 2048 records, 8 bytes a record for the large tier's labels.  Two results
 * come back in between (the clusters, the lists' lengths) and one after every sweep of the large tier; returns after the
 * stream has drained.  stage_ms is a diagnostic (tools/optical_probe.py): the wall time of the three parts the call's own
 * waits cut it into, launches and waits included. */
#define FQD_OPTICAL_MAX_CLUSTER 65536u
#define FQD_PLACE_SAME_SURFACE 0x80000000u
enum fqd_place_reason {
    FQD_PLACE_OK = 0,
    FQD_PLACE_FEW_FIELDS = 1,    /* W has fewer than seven fields */
    FQD_PLACE_EMPTY_FIELD = 2,   /* one of the first seven fields is empty */
    FQD_PLACE_NOT_DIGIT = 3,     /* tile or x holds a byte that is no digit, or y does not begin with one */
    FQD_PLACE_TOO_LONG = 4,      /* tile or x has more than nine digits, or y begins with more than nine */
    FQD_PLACE_BAD_END = 5        /* y's digits are followed by a byte other than ':' '_' '#' '/' */
};
typedef struct fqd_places_info {
    uint64_t bad_record;
    uint32_t bad_reason;        /* enum fqd_place_reason */
    uint32_t reserved;
    uint64_t other_surface;
} fqd_places_info;
typedef struct fqd_optical_info {
    uint64_t clusters_in;
    uint64_t clusters_out;
    uint64_t split;
    uint32_t largest;
    uint32_t sweeps;
    uint32_t max_cluster;
    uint32_t over_limit_members;
    uint64_t over_limit_first;
    float    stage_ms[4];       /* host wall time between the call's own synchronisations: heads + classes, the tiers up to a workgroup, the large tier; 0 */
} fqd_optical_info;
int  fqd_read_places(fqd_engine* e, const uint8_t* text, const uint64_t* id_start, const uint32_t* id_len, uint64_t n, uint32_t* tile, uint32_t* x,
                     uint32_t* y, uint32_t* surface, fqd_places_info* info);
int  fqd_optical_split(fqd_engine* e, const uint32_t* perm, const uint8_t* head, const uint8_t* text, const uint64_t* id_start, const uint32_t* tile,
                       const uint32_t* x, const uint32_t* y, const uint32_t* surface, uint64_t n, uint32_t distance, uint32_t* owner_out,
                       fqd_optical_info* out);

/* ---- FQD_FAST_HAMMING=D: exact clusters within D substituted bases of one another are one cluster (added within ABI version 5:
 * purely additive; no existing entry launches anything new).  Rule and proofs: csrc/fqd_near_core.hpp.  A node is one exact
 * cluster (a record with owner[i] == i) with the shape (len1) or (len1, len2).  Two nodes are near when their shapes are equal,
 * their mates 1 differ in at most D byte positions and, for pairs, their mates 2 differ in at most D positions as well; 'N' is a
 * letter like any other.  A merged cluster is a connected component of that relation, owned by its first record in input order.
 *
 * fqd_near_merge: device memory only (out: host, not NULL).  reads = the engine's segments (1 or 2), ragged or uniform, over
 * n < 2^31 records; owner = fqd_owners' over the same records.  distance = D, 1 .. 3 (anything else: FQD_ERR_ARG); flags = 0 or
 * FQD_NEAR_WEAK_SEEDS.  owner_out[i] (n uint32) = the first record of record i's merged cluster; fqd_group_owners and
 * fqd_owners_to_keep take it.  owner_out must not overlap owner, a segment's offsets or lengths, or the bases of a uniform
 * segment (FQD_ERR_ARG).  An owner above its record, or one that is not its own owner, is FQD_ERR_ARG (counted on the device,
 * nothing written).  Mate 1 of every node is cut into D + 1 segments at floor(j * len / (D + 1)); a node's entry for segment j is
 * (a 64-bit hash of shape, j and the segment's bytes; the node), and two near nodes share a key.  The entries are sorted by key
 * (the radix passes of the ID join); within a group of equal keys every pair of entries of two different nodes is compared byte
 * for byte over both mates, eight lanes a pair and sixteen bytes a lane, and a pair that is near is an edge; min-label sweeps
 * with pointer jumping over the edge list give the components.  *out: nodes; merged = the merged clusters (nodes - merged exact
 * clusters went into another); entries = nodes * (D + 1); groups = the seed groups; pairs = the pairs compared; edges = the
 * pairs found near (a pair that shares several seeds is counted once for each); largest_group = the entries of the largest
 * group; sweeps = the label sweeps (a sweep = a min step that changed a label, and the pointer jump behind it); max_group =
 * FQD_NEAR_MAX_GROUP.  A group of more entries than that is refused: over_limit_first = the lowest first record among the nodes
 * of such a group (FQD_UMI_NO_RECORD: there is none), over_limit_nodes = that group's entries; the call returns FQD_OK,
 * owner_out is unspecified, and merged, pairs, edges and sweeps are 0.  FQD_NEAR_WEAK_SEEDS (tests) cuts every key to its low 4
 * bits: nodes that agree on nothing meet in one group, a node's own entries among them, and the result is the same.  Scratch
 * during the call: 24 bytes an entry for the sort, 4 bytes a record for the labels (owner_out holds the second label array) and
 * 8 bytes an edge; the edge list starts with room for `entries` edges (FQD_NEAR_EDGE_ROOM=K in the environment: for K) and, where
 * the verification counts more, is made as large as the count and the verification runs once more.  Results come back after the
 * node count, the groups, each verification and every sweep; returns after the stream has drained.  stage_ms is a diagnostic
 * (tools/near_probe.py): the wall time of seeds + sort + groups, of the verification and of the sweeps, launches and waits
 * included. */
#define FQD_NEAR_MAX_GROUP 4096u
#define FQD_NEAR_WEAK_SEEDS 1u    /* test hook: seed keys cut to their low 4 bits */
typedef struct fqd_near_info {
    uint64_t nodes, merged, entries, groups, pairs, edges, largest_group, sweeps, over_limit_first, over_limit_nodes;
    uint32_t max_group, reserved;
    float    stage_ms[3];
} fqd_near_info;
int  fqd_near_merge(fqd_engine* e, const fqd_reads* reads, const uint32_t* owner, uint64_t n, uint32_t distance, uint32_t flags,
                    uint32_t* owner_out, fqd_near_info* out);

/* ---- FQD_FAST_UMI_HAMMING=D: exact clusters under ONE UMI within D substituted bases of one another are one molecule (added
 * within ABI version 5: purely additive; no existing entry launches anything new, fqd_near_merge among them).  Rule and proofs:
 * csrc/fqd_near_umi_core.hpp.  A node is one exact cluster of the run keyed B(U) ‖ mate 1, mate 2 (owner[i] == i).  Its tag T(U)
 * is the umi_len bytes of its first record's UMI field with every joiner place set to 0; with the run's one shape, equal tags
 * are equal B(U).  Two nodes are near when their tags are equal and they are near by fqd_near_merge's rule (equal shapes, at most
 * D differing byte positions a mate).  With link, every node v is also joined to link[v].  A molecule is a connected component of
 * the two relations, owned by its first record in input order.
 *
 * fqd_near_merge_umi: device memory only (info, out: host, not NULL).  reads, owner, n, distance, flags and owner_out are
 * fqd_near_merge's: reads = the sequences as they lie in the files, NOT the keyed `UMI bases ‖ sequence` bytes.  text, id_start,
 * umi_off and info are fqd_umi_find's over file 1 and the same n records; an info that names a refused record, or a umi_len
 * outside 1 .. 64, is FQD_ERR_ARG.  link (n uint32, or NULL for no links) = fqd_umi_merge's owner_out over the same owners: only
 * its entries at nodes are read; a link[v] above v, or one that is no node, is FQD_ERR_ARG (counted on the device, nothing
 * written).  owner_out must not overlap owner, link, id_start, umi_off or what fqd_near_merge names.  A node's seed keys are
 * fqd_near_merge's with the ceil(umi_len / 8) little-endian words of its tag absorbed in front of the segment's bytes, so that
 * one sequence under many UMIs is many groups of one; the verification compares the tags byte for byte, lane gl of a pair's
 * eight lanes tag word gl, before shapes and mates.  No load leaves U.  (link[v], v) of every node with link[v] != v stands in
 * the edge list in front of the near edges; the list's room and regrowth cover both.  *out: near = fqd_near_merge's counts, with
 * merged = the molecules and edges = the near edges alone; links = the nodes with link[v] != v.  A seed group beyond
 * FQD_NEAR_MAX_GROUP is refused as in fqd_near_merge.  Scratch and the results that come back are fqd_near_merge's, and one
 * result more (the links) where link is given. */
typedef struct fqd_near_umi_info { fqd_near_info near; uint64_t links; uint64_t reserved; } fqd_near_umi_info;
int  fqd_near_merge_umi(fqd_engine* e, const fqd_reads* reads, const uint32_t* owner, const uint32_t* link /* may be NULL */,
                        uint64_t n, uint32_t distance, uint32_t flags,
                        const uint8_t* text, const uint64_t* id_start, const uint32_t* umi_off, const fqd_umi_info* info,
                        uint32_t* owner_out, fqd_near_umi_info* out);

/* ---- FQD_FAST_PREFIX=L: exact clusters that are prefixes of another, over at least L bases a mate, are copies of it (added
 * within ABI version 5: purely additive; no existing entry launches anything new).  Rule and proofs: csrc/fqd_prefix_core.hpp.
 * A node is one exact cluster (a record with owner[i] == i); span = len1 + len2.  a is a prefix of b when len1(a) <= len1(b), the
 * bytes of a's mate 1 are the first len1(a) bytes of b's and, for pairs, the same holds for mate 2 (same-sided: a pair with the
 * shorter mate 1 and the longer mate 2 is not related); 'N' is a letter like any other.  A node is eligible when every mate has
 * at least L bytes; a node that is not stays a cluster of its own.  An eligible node's parent is, among the eligible nodes it is
 * a prefix of, the one with the least span and among those the lowest record.  A merged cluster is one tree of the parent
 * relation, owned by its first record in input order: every member is a prefix of the tree's root, and two roots are never in
 * one cluster (this is NOT single linkage).
 *
 * fqd_prefix_merge: device memory only (out: host, not NULL).  reads = the engine's segments (1 or 2), ragged or uniform, over
 * n < 2^31 records; owner = fqd_owners' over the same records.  min_overlap = L, 1 .. 65535 (anything else: FQD_ERR_ARG); flags =
 * 0 or FQD_PREFIX_WEAK_SEEDS.  owner_out[i] (n uint32) = the first record of record i's merged cluster; fqd_group_owners and
 * fqd_owners_to_keep take it.  span_out[i] (n uint32, or NULL) = len1 + len2 of record i: constant on an exact cluster, and its
 * maximum over a merged cluster is the root's alone, so fqd_seq_pick_best over it puts the first copy of the root sequence at
 * the head's place.  Neither may overlap the other, owner, a segment's offsets or lengths, or the bases of a uniform segment
 * (FQD_ERR_ARG).  An owner above its record, or one that is not its own owner, is FQD_ERR_ARG (counted on the device, nothing
 * written); so is a mate of 2^31 bytes or more (a span fits 32 bits).  An eligible node's entry is (a 64-bit hash of paired?, L
 * and the first L bytes of each mate; the node), and related nodes share a key.  The entries are sorted by key (the radix passes
 * of the ID join); within a group of equal keys every pair of entries whose lengths allow a prefix — both mates <=, or both >=,
 * and not one shape — is compared byte for byte over the short node's lengths, eight lanes a pair and sixteen bytes a lane, and
 * a related pair offers (span(long) << 32 | long) to a 64-bit atomicMin at the short node: the parent.  Pointer jumping over the
 * parents gives every node's root, an atomicMin over the nodes the first record of every tree.  *out: nodes; eligible; merged =
 * the merged clusters (trees, and the nodes that are not eligible); groups = the seed groups; pairs = the pairs compared byte for
 * byte; related = those found related; children = the nodes with a parent (nodes - merged); largest_group = the entries of the
 * largest group; deepest = the longest parent chain in links, counted by a walk of every child's chain; jumps = the pointer
 * jumps that changed something, ceil(log2(deepest)); max_group = FQD_PREFIX_MAX_GROUP.  A group of more entries than that is
 * refused: over_limit_first = the lowest first record among the nodes of such a group (FQD_UMI_NO_RECORD: there is none),
 * over_limit_nodes = that group's entries; the call returns FQD_OK, owner_out and span_out are unspecified, and merged, pairs,
 * related, children, deepest and jumps are 0.  FQD_PREFIX_WEAK_SEEDS (tests) cuts every key to its low 4 bits: nodes that agree
 * on nothing meet in one group, and the result is the same.  Scratch during the call: 24 bytes an entry for the sort, 8 bytes a
 * record for the parents (then the trees' first records) and 4 bytes a record for the roots (owner_out holds the second array of
 * the jumps).  Results come back after the counts, the groups, the verification and every jump; returns after the stream has
 * drained.  stage_ms is a diagnostic (tools/prefix_probe.py): the wall time of seeds + sort + groups, of the verification and of
 * the trees, launches and waits included. */
#define FQD_PREFIX_MAX_GROUP 4096u
#define FQD_PREFIX_WEAK_SEEDS 1u   /* test hook: seed keys cut to their low 4 bits */
typedef struct fqd_prefix_info {
    uint64_t nodes, eligible, merged, groups, pairs, related, children, largest_group, deepest, jumps, over_limit_first, over_limit_nodes;
    uint32_t max_group, reserved;
    float    stage_ms[3];
} fqd_prefix_info;
int  fqd_prefix_merge(fqd_engine* e, const fqd_reads* reads, const uint32_t* owner, uint64_t n, uint32_t min_overlap, uint32_t flags,
                      uint32_t* owner_out, uint32_t* span_out /* may be NULL */, fqd_prefix_info* out);

/* ---- FQD_FAST_CONSENSUS=1: the written member of every cluster carries the cluster's consensus (added within ABI version 5:
 * purely additive; no existing entry launches anything new).  Rule and proofs: csrc/fqd_consensus_core.hpp.  A cluster is a run
 * of (perm, head); its written member is perm[head place].  In every column p of a cluster of two or more members each member
 * votes for its base with the weight of its quality byte (q - 33 for q >= 33, else 0; 0 for a base that is none of A, C, G, T,
 * which stands for N).  The present letter with the largest sum wins — among tied letters the written member's own, else the
 * first of A, C, G, T, N — and its quality is the winner's sum minus all other sums, clamped to 0 .. 93, written as 33 + Q.
 *
 * fqd_consensus: device memory only (info: host, not NULL), called once per file (mate) over that file's text and record arrays
 * (fqd_scan_records': record r is the size[r] bytes at text + start[r], its sequence line the seq_len[r] bytes at text +
 * seq_off[r], its quality line the seq_len[r] bytes at text + start[r] + size[r] - 1 - seq_len[r]).  (perm, head) =
 * fqd_group_owners' over the current owners, after fqd_seq_pick's exchange where the best member is written.  The seq_len
 * sequence bytes and seq_len quality bytes of the written member of every cluster of two or more are replaced where they
 * lie: a sequence byte only where the winner is not the member's own letter, every quality byte.  No other byte of the text
 * is stored to: ID lines, '+' lines, newlines, the other members and clusters of one stay as they are.  The result does not
 * depend on how the members are dealt to lanes and workgroups, nor on the order of atomics: two calls on equal inputs give
 * equal bytes.  *info: clusters = the clusters of two or more members; members = the records read for them; bases_changed =
 * the columns whose winner is not the written member's own letter; reads_changed = the written records with at least one
 * such column; largest = the members of the largest cluster (of one, too).
 * changed (device, n bytes by record, or NULL): how a paired run counts its pairs once.  The call sets changed[r] = 1 for
 * every written record r it counts in bases_changed, and counts in reads_changed only those whose byte was 0 before.  The host
 * zeroes the array, hands it to the calls over file 1 and file 2, and adds the two calls' reads_changed (the pairs changed in
 * either mate) and bases_changed.  NULL: reads_changed counts every written record of this call with a changed column.
 * FQD_ERR_ARG, with NOTHING stored to the text: n >= 2^31; flags other than 0 or FQD_CONSENSUS_SMALL_TIERS; head[0] == 0 or an
 * order that names a record outside 0 .. n-1; a record (any, of a cluster of one as well) whose quality line does not lie
 * behind its sequence line inside the record (size < seq_len + 1, seq_off < start, or seq_off + seq_len not below the quality
 * line's start: the records of a FASTA file); members of one cluster with different seq_len.  All of it is counted on the
 * device in the first launch.
 * Clusters go by size: up to 64 members — sixteen lanes, four columns a lane and load, the members one after the other; up to
 * 2^20 - 1 — a workgroup whose four waves take every fourth member and combine their columns' states in LDS; from 2^20 on —
 * up to 2048 workgroups a cluster add 64-bit sums and presence masks with atomics to 48 bytes a column of scratch, and a second
 * launch stores the result, one such cluster after the other.  FQD_CONSENSUS_SMALL_TIERS (tests) lowers the two bounds to 8
 * and 64 members and a workgroup's share of a larger cluster from 4096 members to 16.  Sums are 32-bit where the tier bounds
 * the members to 2^20 (222 * 2^20 < 2^28), 64-bit beyond.  No load leaves a line (a line's last, partial four bytes go byte by
 * byte), and every store to the written member's row comes after the last read of it (csrc/fqd_consensus.hip).  Scratch during
 * the call: 4 bytes a cluster, about 4.2 bytes a record for the lists, 48 bytes a column of the longest read where n >= 2^20.
 * Two results come back in between (the clusters and checks, the lists' lengths); returns after the stream has drained. */
#define FQD_CONSENSUS_SMALL_TIERS 1u    /* test hook: tier bounds of 8 and 64 members, 16 members a workgroup beyond */
typedef struct fqd_consensus_info { uint64_t clusters;      /* clusters of >= 2 members */
                                    uint64_t members;       /* records read for them */
                                    uint64_t bases_changed; /* columns whose winner is not the written member's own letter */
                                    uint64_t reads_changed; /* written records with at least one such column */
                                    uint64_t largest; } fqd_consensus_info;
int  fqd_consensus(fqd_engine* e, const uint32_t* perm, const uint8_t* head, uint64_t n, uint8_t* text, const uint64_t* start, const uint32_t* size,
                   const uint64_t* seq_off, const uint32_t* seq_len, uint32_t flags, uint8_t* changed, fqd_consensus_info* info);

/* ---- FQD_FAST_CENTROID=abundant: the most abundant sequence of every cluster (csrc/fqd_centroid_core.hpp) --------------------
 * A merged cluster (FQD_FAST_UMI_MISMATCH, _HAMMING, _UMI_HAMMING, FQD_FAST_OPTICAL on top of them) is a union of exact
 * clusters.  (perm, head) = fqd_group_owners' over the final owners: a run is a cluster, its members in input order.
 * label[r] (device, n uint32 by record) = record r's exact owner, fqd_owners' over the run's exact keys.  The SUB-CLUSTER of a
 * member is the members OF ITS RUN with its label — a label may stand in several runs, behind an optical split — and its
 * abundance the sum of their weights (weight: device, n uint32 by record, NULL: 1 each), summed in 64 bits and stored as
 * min(sum, 2^32 - 1).  A weighted cluster above 2^31 - 1 ends a run in fqd_cluster_weights before any output exists, so a
 * saturated value never decides an output.
 *
 * fqd_subcluster_sizes: abundance[r] (device, n uint32 by record, like fqd_seq_scores' scores) = that sum for every record r,
 * each entry stored exactly once, nothing else stored to.  Device memory only (info: host, may be NULL); n < 2^31.
 * fqd_seq_pick_best(e, abundance, head, n, perm, &moved) then puts every cluster's centroid — the first member of the
 * sub-cluster of the largest abundance, of equal ones the one whose first member stands earliest — at the head's place;
 * moved = the clusters written by another sequence than their first member's.  The result does not depend on how members
 * are dealt to lanes and workgroups nor on the order of atomics.  *info: clusters; mixed = those of two or more
 * sub-clusters; subclusters = all of them; tier_clusters = the clusters of one member, of up to 8 (eight lanes a cluster),
 * up to 64 (a wave), up to 2048 (a workgroup, its labels in a table in LDS) and above (many workgroups a cluster and a table
 * in scratch keyed (head place << 32 | label); no upper limit and no refusal); largest = the members of the largest cluster.
 * FQD_ERR_ARG, with NOTHING written: n >= 2^31 (before anything is allocated); abundance overlapping an input; head[0] == 0,
 * an order that names a record outside 0 .. n-1 or a label outside 0 .. n-1 — counted on the device in the first launch and
 * reported once.  n = 0: FQD_OK without a launch.  Scratch during the call: 4 bytes a cluster, about 5 bytes a record for
 * the lists, and 32 bytes a member of the clusters above 2048.  Two results come back in between (the clusters and checks,
 * the lists' lengths); returns after the stream has drained.
 *
 * fqd_subcluster_scores, behind that pick, for FQD_FAST_KEEP=best INSIDE the winning sub-cluster: masked[r] (device, n uint32
 * by record) = min(score[r], 2^32 - 2) + 1 where label[r] is the label of the record at the head place of r's run, 0
 * elsewhere; every entry stored exactly once.  A second fqd_seq_pick_best over masked puts the best-scored copy of the most
 * abundant sequence at the head's place, the earliest in the input among equals (the centroid stands at the head, the
 * other copies of its sequence in input order behind it).  Same memory rules and FQD_ERR_ARG cases as above, without the
 * labels' range (they are only compared); scratch: 4 bytes a tile of 2048 places; returns after the stream has drained. */
typedef struct fqd_centroid_info {
    uint64_t clusters, mixed /* clusters of >= 2 sub-clusters */, subclusters;
    uint64_t tier_clusters[5];   /* one member, <= 8, <= 64, a workgroup's, above */
    uint32_t largest, reserved;
} fqd_centroid_info;
int  fqd_subcluster_sizes(fqd_engine* e, const uint32_t* perm, const uint8_t* head, const uint32_t* label,
                          const uint32_t* weight /* NULL: 1 each */, uint64_t n, uint32_t* abundance, fqd_centroid_info* info /* host, may be NULL */);
int  fqd_subcluster_scores(fqd_engine* e, const uint32_t* perm, const uint8_t* head, const uint32_t* label,
                           const uint32_t* score, uint64_t n, uint32_t* masked);

/* keep_out[origin[k]] = flags[k] for k < n: puts the flags that came back from the
 * owners (in partition order) into input order.  All device pointers. */
int  fqd_scatter_flags(fqd_engine* e, const uint8_t* flags, const uint32_t* origin, uint64_t n, uint8_t* keep_out);

/* ---- synthetic workload (bench.py, tests): SURVEY §8(d) ---------------------
 * Fills `bases` (device) with n reads of `len` bases at stride `len`, global
 * indices [first, first+n): read g>0 is with probability dup_permille/1000 a
 * copy of a uniformly chosen earlier read (chains allowed), else fresh uniform
 * ACGT (one N in about 1 read of 8).  mate = 0/1 selects the mate stream of a
 * pair; for mate 1 a copied pair keeps its parent's mate-2 with probability 1/2.
 * expect_keep (device, may be NULL) receives the analytically known flags. */
int  fqd_synth_reads(fqd_engine* e, uint64_t seed, uint64_t first, uint64_t n, uint32_t len,
                     uint32_t dup_permille, int mate, uint8_t* bases, uint8_t* expect_keep);

#ifdef __cplusplus
}
#endif
#endif /* FQDUPAWAY_H */
