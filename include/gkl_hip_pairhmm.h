/*
 * gkl_hip_pairhmm.h -- C ABI of the MI355X-native PairHMM forward hot path.
 *
 * This is the drop-in boundary.  Everything below is plain C: pointers, sizes and
 * status codes -- no JNI, no torch, no C++ types.  The JNI symbols that GKL's Java
 * class com.intel.gkl.pairhmm.IntelPairHmm binds (libgkl_pairhmm.so, see
 * include/gkl_pairhmm_jni.h) are thin shims over these entry points, and so is
 * the ctypes binding in gkl_amd/native.py.
 *
 * What each entry point replaces in the reference (paths under
 * /root/reference/src/main/native/pairhmm):
 *
 *   gklhip_init            initNative: IntelPairHmm.cc:55-118 (globals g_use_double,
 *                          g_max_threads, FTZ, kernel choice) + the static Context<T>
 *                          table objects of IntelPairHmm.cc:44-45 / Context.h:133-189
 *   gklhip_compute         computeLikelihoodsNative after marshalling:
 *                          IntelPairHmm.cc:150-169 (batch loop, fp32->fp64 policy,
 *                          log10) calling compute_full_prob_* of
 *                          avx-pairhmm-template.h:235-372
 *   gklhip_compute_device  same, with the batch already resident in HBM
 *   gklhip_done            doneNative: IntelPairHmm.cc:189-192
 *   gklhip_init_devices    same as gklhip_init for a LIST of devices: every call is then cut into contiguous
 *                          read ranges balanced by cells, one per device -- what the reference's OpenMP
 *                          `schedule(dynamic,1)` loop over pairs (IntelPairHmm.cc:151-154) is to its cores
 *
 * The flat batch replaces the std::vector<testcase> that JavaData::getData builds
 * (JavaData.h:65-111; testcase = pairhmm_common.h:43-47): reads x haplotypes cross
 * product, r-major, result index r*n_haps + h (JavaData.h:94-105, IntelPairHmm.cc:167).
 */
#ifndef GKL_HIP_PAIRHMM_H
#define GKL_HIP_PAIRHMM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GKLHIP_ABI_VERSION 2

typedef struct gklhip_ctx gklhip_ctx; /* opaque; one per initNative */

typedef enum {
  GKLHIP_OK = 0,
  GKLHIP_ERR_INVALID_ARG = 1, /* -> java/lang/IllegalArgumentException */
  GKLHIP_ERR_NO_DEVICE = 2,   /* no usable gfx950 device: fails loudly, no CPU fallback */
  GKLHIP_ERR_OOM = 3,         /* -> java/lang/OutOfMemoryError */
  GKLHIP_ERR_HIP = 4,         /* any other HIP runtime failure -> java/lang/RuntimeException */
  GKLHIP_ERR_UNSUPPORTED = 5
} gklhip_status;

/* How raw kernel sums become log10 likelihoods (IntelPairHmm.cc:159-165). */
typedef enum {
  /* Exactly the reference's arithmetic, evaluated on the HOST with the host libm:
   * fp32 pairs (double)(log10f(raw) - log10f(2^120)), fp64 pairs
   * log10(raw) - log10(2^1020).  Bit-identical to GKL given bit-identical sums.
   * Default of gklhip_compute (host buffers). */
  GKLHIP_FINALIZE_REFERENCE_HOST = 0,
  /* Evaluated on the device in double: log10((double)raw) - log10(2^{120|1020}).
   * Never further from the reference's fp64 path than the fp32 recurrence itself
   * (the reference's log10f adds up to 3.8e-6 absolute). Default of
   * gklhip_compute_device. */
  GKLHIP_FINALIZE_DEVICE_F64 = 1,
  /* Device emulation of the reference formula: float-rounded log10 and float
   * subtraction; within 1 float ulp (3.8e-6) of GKLHIP_FINALIZE_REFERENCE_HOST. */
  GKLHIP_FINALIZE_DEVICE_REF32 = 2
} gklhip_finalize;

typedef struct {
  int32_t abi_version;  /* GKLHIP_ABI_VERSION */
  int32_t device;       /* HIP device ordinal, -1 = current device */
  int32_t use_double;   /* PairHMMNativeArguments.useDoublePrecision (IntelPairHmm.cc:70) */
  int32_t max_threads;  /* maxNumberOfThreads (IntelPairHmm.cc:72-89): a CAP on the host threads of the reference-exact
                           finalize, honoured as given -- 1 (the reference's default) = one thread per call;
                           <= 0 = not set: the calls in flight share min(cores, 8).  GKL_HIP_FINALIZE_THREADS overrides */
  int32_t fma_mode;     /* 1 = arithmetic of GKL's AVX-512 objects (gcc-contracted FMA; default),
                           0 = arithmetic of GKL's AVX objects (separate mul/add) */
  int32_t finalize;     /* gklhip_finalize for gklhip_compute_device; -1 = default */
  int32_t record_events;/* 1 = bracket kernels with HIP events and synchronise every call (gklhip_get_stats);
                           2 = record into a ring of 64 event sets WITHOUT synchronising: calls pipeline, the
                               times are read afterwards with gklhip_get_step_times */
  int32_t rows_per_lane;/* fp32 main kernel: 0 = auto (8 rows per lane; 4 or 2 for small batches), 8 = 8-row kernel,
                           4 (or -4) = 4-row kernel, 2 = 2-row kernel when every read has at most 127 bases, else 4 */
} gklhip_config;

/* Flat structure-of-arrays batch. Offsets always live on the host; the byte
 * arrays live on the host for gklhip_compute and in HBM for gklhip_compute_device.
 * Quals are raw Phred bytes; they are masked with &127 like
 * avx-pairhmm-template.h:134-136,149. */
typedef struct {
  int32_t n_reads;
  int32_t n_haps;
  const int64_t* read_off;   /* [n_reads+1], read_off[0] == 0 */
  const int64_t* hap_off;    /* [n_haps+1],  hap_off[0] == 0 */
  const uint8_t* read_bases; /* [read_off[n_reads]]  ReadDataHolder.readBases    */
  const uint8_t* read_quals; /*                      ReadDataHolder.readQuals    */
  const uint8_t* ins_gop;    /*                      ReadDataHolder.insertionGOP */
  const uint8_t* del_gop;    /*                      ReadDataHolder.deletionGOP  */
  const uint8_t* gcp;        /*                      ReadDataHolder.overallGCP   */
  const uint8_t* hap_bases;  /* [hap_off[n_haps]]    HaplotypeDataHolder.haplotypeBases */
} gklhip_batch;

typedef struct {
  int64_t n_pairs;
  int64_t n_fallback;      /* pairs recomputed in fp64 (raw fp32 sum < 1e-28f) */
  int64_t cells;           /* sum of rslen*haplen over all pairs */
  int64_t cells_fp64;      /* same over the fp64-recomputed pairs */
  int32_t n_chunks;        /* 64-lane read packs of the fp32 (or all-fp64) pass */
  int32_t n_hap_groups;
  int32_t rows_per_lane;
  int32_t n_long_pairs;    /* pairs of the main pass routed to the striped long-read kernel */
  float ms_fwd_main;       /* HIP-event time of the main forward kernel (record_events) */
  float ms_fwd_fallback;   /* HIP-event time of the fp64 fallback kernel */
  float ms_total_device;   /* first launch .. last kernel of the call */
  float lane_fill;         /* useful rows / (chunks * 64 * rows_per_lane) of the main pass */
} gklhip_stats;

/* Lifecycle.  gklhip_init uses cfg->device; when that is -1 and the environment names a list
 * (GKL_HIP_DEVICES=0,1,2,...), it is gklhip_init_devices with that list. */
int gklhip_init(const gklhip_config* cfg, gklhip_ctx** out_ctx);
int gklhip_done(gklhip_ctx* ctx);

/* One context over several devices of this node, driven by this one process (one host thread per extra device).
 * Every call is sharded by contiguous read ranges balanced by cells (gklhip_partition_reads), haplotypes and tables
 * replicated.  gklhip_compute: each device copies its range from the caller's host arrays and its results back over
 * its own PCIe link -- no device-to-device step.  gklhip_compute_device: inputs and the output array live on
 * devices[0]; the other devices pull their ranges over xGMI and their results are gathered into the output array --
 * with RCCL (ncclCommInitAll + one ncclSend/ncclRecv pair per device in one group; librccl.so is dlopen()ed by the
 * first multi-device context) when the devices are distinct, with peer copies otherwise (a device may be listed
 * twice: two shards on one GPU, what the one-GPU tests do).  GKL_HIP_GATHER=peer|rccl overrides the choice.
 * devices == NULL or n_devices <= 0: cfg->device alone. */
int gklhip_init_devices(const gklhip_config* cfg, const int32_t* devices, int32_t n_devices, gklhip_ctx** out_ctx);
int gklhip_num_devices(gklhip_ctx* ctx);
/* 0 = single device (no gather), 1 = peer copies, 2 = RCCL (before the first device-resident call: what that call
 * will try -- the communicators are created lazily), 3 = peer copies because RCCL failed (library missing, a device
 * listed twice, ncclCommInitAll or a group call returning an error; gklhip_gather_note says which).  An RCCL failure
 * never fails a call: the shards' results are gathered with peer copies instead, bit-identically.
 * GKL_HIP_RCCL_FAIL=init|group forces such a failure (tests). */
int gklhip_gather_backend(gklhip_ctx* ctx);
const char* gklhip_gather_note(gklhip_ctx* ctx);
/* The sharding rule: bounds_out[0] = 0 <= ... <= bounds_out[n_parts] = n_reads, contiguous read ranges whose summed
 * read lengths (= cells, every range meets every haplotype) are as equal as cut points between reads allow. */
int gklhip_partition_reads(int32_t n_reads, const int64_t* read_off, int32_t n_parts, int32_t* bounds_out);
/* Diagnostics: dlopen RCCL and run the gather's send/recv group on a one-device communicator.  0 = ok. */
int gklhip_rccl_selftest(int32_t device);

/* Host buffers in, host doubles out (n_reads*n_haps). What the JNI shim calls.  The byte arrays
 * are copied to the device asynchronously; when they live in memory from gklhip_host_alloc the
 * copies are true DMA (no bounce through the runtime's staging pages).  Results come back as one
 * 8-byte word per pair through pinned memory owned by the context. */
int gklhip_compute(gklhip_ctx* ctx, const gklhip_batch* host_batch, double* out_host);

/* Several region calls, the GATK-sized ones in ONE set of launches: region k's output is, byte for byte, what
 * gklhip_compute(ctx, &regions[k], out_host[k]) writes on the same context -- whichever other regions ride along, in
 * whatever order, in both fma modes.  out_host: [n_regions] pointers, region k's n_reads * n_haps doubles.  status_out:
 * [n_regions] or NULL.
 * Returns GKLHIP_OK when every region succeeded, else the status of the first failing region (gklhip_last_error: its
 * message); the per-region statuses are in status_out and the regions that succeeded have valid results.  The argument
 * checks of the single call run per region before anything touches the device: a region that fails them is left out and
 * the rest still run.  A region with n_reads * n_haps == 0 succeeds and writes nothing.  A HIP failure of a shared set of
 * launches fails every region in that set (after its stream has been drained).
 * Which regions share a set: SMALL ones, those the single call hands to the small-call combiner (inputs of at most 1 MB,
 * at most 2048 pairs, no read beyond the small-read limit -- 383 bases, or 511 with GKL_HIP_SMALL_READ_LIMIT=511 /
 * gklhip_set_small_read_limit --, host finalisation, no record_events), and MID-SIZE
 * ones, for which all of that holds except the size: 2049 to 65 536 pairs.  The two are cut apart.  The small regions,
 * in input order, are cut into sets of one kind (with rows_per_lane == 0: the fused per-pair kernel) of at most 64
 * regions.  Small calls come in kinds, and a set -- of a multi call or of concurrent callers -- holds one kind only: the
 * fused per-pair kernel, the fp32 pass + per-pair policy (rows_per_lane != 0), and, on a use_double context, the
 * all-fp64 per-pair kernel (every pair in double precision, one pair per wavefront; its size limit is the same 2048
 * pairs, kSmallDoublePairs; rows_per_lane, an fp32 setting, does not matter there).  A context has one precision, so the
 * regions of one multi call never mix; callers on contexts of different precision never share a set.  The mid-size
 * regions share sets among themselves only -- prep, the packed fp32 pass, and the per-pair policy in two launches, once
 * for the whole set; on a use_double context prep, the packed fp64 pass and the packed words of its sums: three launches,
 * and there the read-length limit is the chunk of that pass, 639 bases -- in input order, at most 64 per set, and they need company of their
 * own kind: ONE mid-size region in a call is no set and runs alone, as before.  Each region of a set is planned and staged
 * exactly as a single call is, on one of up to 64 staging lanes of the context (made on first use, given back by
 * gklhip_release_idle), and a set leaves through the combiner's launches: it waits for a flight slot like the set of any
 * concurrent callers, but takes nobody else's calls and waits for no company.  Every other region -- and every region of
 * a multi-device context, of a process with GKL_HIP_COMBINE=0 and of a client context, whose wire protocol has no multi
 * request -- is computed afterwards through the single-call path, in input order.  A single gklhip_compute of a mid-size
 * region -- and a region of a multi call that runs through the single-call path -- is combined with nothing unless the
 * context's mid-size switch is on (gklhip_set_mid_combine, below; off by default).
 * Memory: a lane keeps the buffers of the biggest region it staged until gklhip_release_idle.  One that held a
 * 65 536-pair region keeps at most about 7 MB of device memory (two plan blocks of up to 1 MB, the haplotype streams,
 * 4 + 8 + 1 bytes per pair of raw sums and flags, the 4 bytes per pair of its list of flagged pairs, its lane map; each
 * allocated a quarter above its size) and 3 MB of pinned host memory (two staging blocks, 8 bytes per pair of result
 * words): 64 such lanes under 0.5 GB and 0.2 GB.  A lane that only ever held 100 x 10 regions keeps a few hundred KB.
 * gklhip_small_call_counts: a set of n regions adds n to the calls, n to the combined calls when n > 1, and 1 to the
 * sets; a region that ran alone counts as a single call does.  Afterwards gklhip_get_stats holds the sums over the
 * regions of n_pairs, n_fallback, cells and cells_fp64 (the other fields are 0), gklhip_get_raw fails ("no completed call
 * to read back": it has no one call to read) and gklhip_get_raw_region reads one region. */
int gklhip_compute_multi(gklhip_ctx* ctx, int32_t n_regions, const gklhip_batch* regions, double* const* out_host,
                         int32_t* status_out);

/* Page-locked host memory for a binder's marshalling buffers (replaces the per-array
 * Get<T>ArrayElements pins of JavaData.h:135-154 with one flat, DMA-able staging area that is
 * reused across calls).  NULL on failure.  Not tied to a context.  In a process with GKL_HIP_SERVER set (client mode,
 * decided at the first call) this is plain memory: such a process makes no HIP call. */
void* gklhip_host_alloc(size_t bytes);
void gklhip_host_free(void* p);

/* Byte arrays and `out_dev` in HBM; launches on `hip_stream` (a hipStream_t; NULL = HIP's
 * default stream) and returns without a host sync when record_events == 0 (the fp64
 * recomputation pass is planned on the device).  The context's scratch is ordered by that stream; a
 * call on a different stream than the previous one first waits (on the device) for that one's end. */
int gklhip_compute_device(gklhip_ctx* ctx, const gklhip_batch* dev_batch, double* out_dev,
                          void* hip_stream);

/* gklhip_compute_multi for regions that are resident in HBM: dev_regions[k] is exactly a `dev_batch` of
 * gklhip_compute_device (offsets on the host, the six byte arrays in HBM on the context's device, at any alignment),
 * `out_dev` a HOST array of n_regions HBM pointers -- region k gets n_reads * n_haps doubles --, status_out [n_regions]
 * or NULL.  No byte of the regions' arrays is copied or read by the host.
 * Results: out_dev[k] is, byte for byte, what gklhip_compute_device(ctx, &dev_regions[k], out_dev[k], ...) writes on the
 * same context -- whichever regions ride along, in whatever order, in both fma modes, in both device finalisation modes
 * (cfg.finalize 1 or 2; anything else means GKLHIP_FINALIZE_DEVICE_F64, as in the single call) and on use_double contexts.
 * Which regions share a set: the rule of gklhip_compute_multi with "arrays in HBM" standing where "inputs inline" stands
 * -- the six arrays of at most 1 MB; small regions (at most 2048 pairs) cut into sets by kind, mid-size regions (2049 to
 * 65 536 pairs; reads of up to 639 bases on a use_double context) among themselves, one alone is no set; the same lanes,
 * flight slots and caps.  The read-length limit of the small-call path is 383 bases in this call whatever
 * gklhip_set_small_read_limit says: the 511-base tier is not offered here.  Every other region, every region of a
 * multi-device context, of a process with GKL_HIP_COMBINE=0 and of a context with record_events != 0 runs through the path
 * of gklhip_compute_device on `hip_stream`, in input order.
 * Ordering: the call is SYNCHRONOUS, and there is no asynchronous variant.  Every set is ordered behind everything already
 * enqueued on `hip_stream` (a set's own stream waits for an event recorded there), and the call returns after all its
 * work has finished, the region-by-region work included.
 * Errors: the argument checks of gklhip_compute_device run per region before anything touches the device (a NULL
 * out_dev[k] is a NULL output array); a region that fails them is left out, its out_dev[k] stays untouched, and the rest
 * run.  Return value and gklhip_last_error are the first failing region's.  A HIP failure of a shared set fails every
 * region of that set after its stream has drained.  A client context returns GKLHIP_ERR_UNSUPPORTED before anything else.
 * Afterwards: gklhip_small_call_counts counts as after gklhip_compute_multi (a set of n regions: n calls, n combined calls
 * when n > 1, 1 set; a region that ran alone: nothing), gklhip_get_stats holds the sums over the regions of n_pairs,
 * n_fallback (-1 when a region ran alone on a context that is not use_double: its count is not known without reading
 * it back), cells and cells_fp64, gklhip_get_raw_region reads one region, gklhip_get_raw refuses, and
 * gklhip_release_idle gives the lanes back. */
int gklhip_compute_multi_device(gklhip_ctx* ctx, int32_t n_regions, const gklhip_batch* dev_regions, double* const* out_dev,
                                int32_t* status_out, void* hip_stream);

/* Introspection (tests, bench). */
int gklhip_get_stats(gklhip_ctx* ctx, gklhip_stats* out);

/* record_events == 2: HIP-event times (ms) of the call `steps_back` calls ago (0 = the last one; at most 63):
 * main forward kernel, fp64 fallback kernel, whole device pipeline.  Waits for that call to finish. */
int gklhip_get_step_times(gklhip_ctx* ctx, int32_t steps_back, float* ms_main, float* ms_fallback, float* ms_total);
/* Raw sums of the last call, copied to host arrays of n_pairs entries (any may be NULL).
 * raw64 is meaningful where used64 != 0. Synchronises the stream. */
int gklhip_get_raw(gklhip_ctx* ctx, float* raw32, double* raw64, uint8_t* used64);
/* gklhip_get_raw for region `region` of the last gklhip_compute_multi call (arrays of that region's n_pairs entries).
 * The raw sums of a region that shared a set stay on its staging lane until a later set of the same call, the next
 * multi call or gklhip_release_idle takes the lane; a region that failed, was empty or ran alone through the
 * single-call path has none (GKLHIP_ERR_UNSUPPORTED). */
int gklhip_get_raw_region(gklhip_ctx* ctx, int32_t region, float* raw32, double* raw64, uint8_t* used64);
/* Host-built lookup tables exactly as uploaded: which = 0 ph2pr[128],
 * 1 matchToMatch triangle for quals 0..127 [8256], 2 ph2pr/3 [128]. Returns count. */
int64_t gklhip_get_table_f32(int which, float* dst, int64_t cap);
int64_t gklhip_get_table_f64(int which, double* dst, int64_t cap);

/* Host-side work planning only (no device needed): how the reads of a batch would be packed into
 * 64-lane chunks at `rows_per_lane` rows per lane and how many haplotype streams are formed.
 * lanes_out (may be NULL) receives n_chunks*64 pairs {read index or -1, row block}; returns the number
 * of chunks, or a negative status. n_groups_out / n_long_out (may be NULL): stream groups, reads
 * routed to the striped long-read kernel. */
int gklhip_plan_describe(int32_t n_reads, int32_t n_haps, const int64_t* read_off, const int64_t* hap_off,
                         int32_t rows_per_lane, int32_t* lanes_out, int64_t lanes_cap, int32_t* n_groups_out,
                         int32_t* n_long_out);

/* Diagnostics: the VALU issue ceiling of the forward recurrence's instruction mix on the context's first device -- a
 * kernel of nothing but 4 multiplies + 4 fused multiply-adds per cell (fp32, or fp64 with use_double), operands placed
 * so that no op stalls on a register bank, four wavefronts per SIMD on every CU, run for about ms_budget milliseconds.
 * cells_per_s: cells of that mix per second (x 12 FLOP = the ceiling bench.py prints next to the vector peak);
 * clock_ghz (may be NULL): shader cycles counted by the kernel / its duration = the clock sustained under that load. */
int gklhip_measure_issue_ceiling(gklhip_ctx* ctx, int use_double, double ms_budget, double* cells_per_s, double* clock_ghz);

/* Diagnostics: concurrent small host-buffer calls (a GATK region each, from several threads or JNI slots) are launched
 * together when they meet on the device (GKL_HIP_COMBINE).  Process-wide counts for `device`:
 * out[0] calls that took the small-call path, out[1] those of them launched together with other calls, out[2] sets of
 * launches issued.  reset != 0 zeroes the counts after reading.  The qualifying calls of use_double contexts are small
 * calls too and are counted like the fp32 ones (they used to take the general pass and count nothing). */
int gklhip_small_call_counts(int device, int64_t out[3], int reset);

/* The small-read limit: the longest read of a region that takes the small-call path (the fused per-pair kernel, the
 * combiner of concurrent callers, the shared sets of gklhip_compute_multi, in single and in double precision): 383
 * bases, or 511 with GKL_HIP_SMALL_READ_LIMIT=511 / gklhip_set_small_read_limit.  A region with a longer read takes the
 * general pass and runs alone inside a multi call.  max_read_len must be exactly 383 (the default) or 511 -- what one
 * wavefront holds at 6 and at 8 rows per lane; anything else is GKLHIP_ERR_INVALID_ARG.  Takes the context's lock and
 * applies to the calls planned afterwards.  New contexts start from the process's environment, read once:
 * GKL_HIP_SMALL_READ_LIMIT=511 means 511, unset or any other value 383 (how the JNI libraries and the PairHMM server get
 * it).  With 511, what keeps the general pass for reads of 384 to 511 bases is what never takes the small-call path
 * anyway: multi-device contexts, record_events != 0, device-resident calls, GKL_HIP_COMBINE=0; reads of 512 bases or
 * more always do.  A call that holds a read of 384 bases or more does not speculate (GKLHIP_SPECULATE_FP64).  Results
 * are bit for bit the same under both limits.  On a client context of the server: GKLHIP_ERR_UNSUPPORTED (the server's
 * contexts follow the server process's environment). */
int gklhip_set_small_read_limit(gklhip_ctx* ctx, int32_t max_read_len);

/* The mid-size switch (opt-in): with on != 0 a single gklhip_compute of a MID-SIZE region on this context -- 2049 to
 * 65 536 pairs, and everything else gklhip_compute_multi asks of a mid-size region that shares a set: inputs of at most
 * 1 MB, host finalisation, no record_events, no read beyond the small-read limit (use_double: beyond 639 bases),
 * GKL_HIP_COMBINE not 0 -- enters the small-call combiner: it is staged as a multi call stages such a region and leaves
 * in ONE set of launches with the like regions of the threads (contexts) that meet it on the device, through the set
 * kernels of the multi call.  Results are bit for bit those of the switched-off call.
 * What stays: a set holds one kind and one fma mode -- mid-size regions never share with small calls, fp32 never with
 * use_double.  Two caps apply to mid-size sets of concurrent callers: a set holds at most 131 072 pairs (the leader, then
 * the waiting regions in arrival order that still fit; one that does not fit is passed over and leads its own set) and at
 * most 16 calls; and at most two of the combiner's four flight slots carry mid-size sets at a time -- a mid-size call that
 * finds two in the air waits in the queue, where it gains company, so that GATK-sized calls always find a slot (with
 * GKL_HIP_COMBINE_FLIGHTS = 2 or 3: at most min(2, slots - 1); with ONE slot there is none to leave them).
 * GKL_HIP_COMBINE_MIN / GKL_HIP_COMBINE_WAIT_US apply as to small calls.  A call that meets nobody leaves as a set of one
 * through the same kernels, on its context's own stream like any lone call (a one-caller process makes no flight streams).
 * What never enters and keeps the general pass: multi-device contexts, device finalisation, record_events != 0, a context
 * with an asynchronous device-resident call in flight, regions above 65 536 pairs or 1 MB of inputs, client contexts.
 * gklhip_small_call_counts counts such calls like small ones: a lone one adds (1, 0, 1) -- (0, 0, 0) with the switch off.
 * gklhip_get_raw and gklhip_get_stats work as after any single call.  The shared sets of a multi call are unchanged.
 * Takes the context's lock and applies to the calls planned afterwards; every engine and staging lane of the context
 * follows.  New contexts start from the process's environment, read once: GKL_HIP_COMBINE_MID set to a non-zero number
 * means on (how the JNI libraries and the PairHMM server get it).  On a client context of the server:
 * GKLHIP_ERR_UNSUPPORTED (the server's contexts follow the server's GKL_HIP_COMBINE_MID). */
int gklhip_set_mid_combine(gklhip_ctx* ctx, int on);

/* Gives back what an IDLE context holds only for speed: the streams it made for big calls (every stream is a hardware
 * queue the device's scheduler rotates among all processes' -- an idle process should hold one or two, not seven), its
 * twin engines of big host-buffer calls and second engines of two-stream device-resident callers.  Nothing happens while a
 * call is running or work is queued; what went is made again by the first call that needs it.  The JNI library calls
 * this for every slot that has been idle for a second (GKL_HIP_IDLE_RELEASE_MS).  *streams_released: how many streams went. */
int gklhip_release_idle(gklhip_ctx* ctx, int32_t* streams_released);

/* Fault injection for tests of a caller's error handling (the JNI shim retries a failed call once on fresh contexts):
 * spec "compute:N" or "compute:NxK" makes the N-th .. (N+K-1)-th gklhip_compute of the process, counted from this call,
 * fail with GKLHIP_ERR_HIP before any work (output array poisoned with NaN); NULL or "" disarms.  The first gklhip_init of
 * a process arms it from the environment variable GKLHIP_FAULT_INJECT. */
int gklhip_fault_inject(const char* spec);

/* ---- Client mode: one server process per node owns the GPU (gkl_amd/lib/gklhip_server) ----
 * gklhip_connect: a context whose calls are computed by the server listening on the Unix-domain socket `socket_path`.
 * The server makes a context of its own from `cfg` (use_double, max_threads, fma_mode, finalize; device only when it
 * was started without --devices) and runs every call through its gklhip_compute, so the calls of many client
 * processes meet in one process's small-call combiner.  A client process makes no HIP call: batches travel through a
 * shared-memory arena (memfd) the server maps.  gklhip_init with GKL_HIP_SERVER=PATH in the environment is
 * gklhip_connect(PATH, cfg, out_ctx).  On a remote context gklhip_compute, gklhip_compute_multi (region by region), gklhip_get_stats, gklhip_release_idle (no-op)
 * and gklhip_done work; gklhip_compute_device, gklhip_compute_multi_device, gklhip_get_raw, gklhip_get_raw_region, gklhip_get_step_times, gklhip_set_small_read_limit, gklhip_set_mid_combine and gklhip_measure_issue_ceiling
 * return GKLHIP_ERR_UNSUPPORTED, and so does gklhip_fault_inject in a process with GKL_HIP_SERVER set.  A server that
 * has gone away fails the call with GKLHIP_ERR_HIP and a message that names the socket. */
#define GKLHIP_SERVER_PROTOCOL 1
#define GKLHIP_SERVER_MAX_DEVICES 16
typedef struct {
  int32_t protocol;          /* GKLHIP_SERVER_PROTOCOL of the server */
  int32_t pid;               /* the server's process id */
  int64_t calls_served;      /* gklhip_compute calls answered (any status) */
  int64_t calls_failed;      /* ... of them with a status other than GKLHIP_OK */
  int32_t calls_active;      /* calls inside gklhip_compute right now */
  int32_t live_connections;  /* compute connections open right now */
  int64_t connections_total; /* compute connections accepted since the start */
  int64_t arenas_registered; /* arenas mapped and page-locked in place (hipHostRegister): H2D is DMA from the client's pages */
  int64_t arenas_copied;     /* arenas whose calls are copied into the server's own pinned staging (registration failed) */
  int64_t requests_refused;  /* malformed requests, refused hellos and peers of another uid */
  int32_t n_devices;         /* entries used below: the --devices list, or the devices the connections asked for */
  int32_t reserved;
  int32_t device[GKLHIP_SERVER_MAX_DEVICES];          /* device ordinal of each entry */
  int32_t connections[GKLHIP_SERVER_MAX_DEVICES];     /* live compute connections on each entry */
  int64_t small_calls[GKLHIP_SERVER_MAX_DEVICES][3];  /* gklhip_small_call_counts of each entry's device */
} gklhip_server_info;

int gklhip_connect(const char* socket_path, const gklhip_config* cfg, gklhip_ctx** out_ctx);
/* 1 for a context made by gklhip_connect (or gklhip_init under GKL_HIP_SERVER), 0 otherwise. */
int gklhip_is_remote(gklhip_ctx* ctx);
/* Asks the server on `socket_path` for its counters (also the JNI library's load-time probe in client mode). */
int gklhip_server_stats(const char* socket_path, gklhip_server_info* out);

/* Page-locks existing host memory (hipHostRegister) so that gklhip_compute's copies from it are DMA; the server does
 * this to the arena it maps.  gklhip_host_unregister undoes it. */
int gklhip_host_register(void* p, size_t bytes);
int gklhip_host_unregister(void* p);

const char* gklhip_strerror(int status);
/* Thread-local detail message of the last failing call on this thread. */
const char* gklhip_last_error(void);
int gklhip_device_count(void);
int gklhip_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* GKL_HIP_PAIRHMM_H */
