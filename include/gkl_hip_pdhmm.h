/*
 * gkl_hip_pdhmm.h -- C ABI of the MI355X-native PDHMM (partially determined haplotype PairHMM),
 * the "next" row f1 of SURVEY.md section 8 / BASELINE.json config 5.
 *
 * Replaces, in the reference (paths under /root/reference/src/main/native/pdhmm):
 *   gklhip_pdhmm_init     initializeNative: pdhmm-implementation.h:303-322 (ProbabilityCache tables
 *                         of pdhmm-common.h:139-192, engine choice) -- here: tables + device context
 *   gklhip_pdhmm_compute  computePDHMM: pdhmm-implementation.h:361-396 -> computePDHMM_<engine>
 *                         (pdhmm.h:1133-1290), on the padded 1:1 batch IntelPDHMM.computePDHMM passes
 *                         (src/main/java/com/intel/gkl/pdhmm/IntelPDHMM.java:147-186)
 *   gklhip_pdhmm_done     doneNative
 * Arithmetic: GKL's, position by position -- its vector kernels (by default as its AVX-512 object computes, gcc-contracted
 * FMAs; optionally as its AVX2 object does) and its scalar engine for the tail of every batch; see gkl_amd/csrc/pdhmm_kernel.h.
 */
#ifndef GKL_HIP_PDHMM_H
#define GKL_HIP_PDHMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gklhip_pdhmm_ctx gklhip_pdhmm_ctx;

/* status codes are gklhip_status of gkl_hip_pairhmm.h (0 ok, 1 invalid argument, 2 no device,
 * 3 out of memory, 4 HIP error, 5 unsupported) */

typedef struct {
  int32_t batch;             /* number of (read, haplotype) pairs */
  int32_t max_hap_len;       /* row stride of the two haplotype arrays */
  int32_t max_read_len;      /* row stride of the five read arrays */
  const int8_t* hap_bases;   /* [batch][max_hap_len] */
  const int8_t* hap_pdbases; /* [batch][max_hap_len] PD flag bytes: SNP 1, DEL_START 2, DEL_END 4, A 8, C 16, G 32, T 64 */
  const int8_t* read_bases;  /* [batch][max_read_len] */
  const int8_t* read_qual;
  const int8_t* read_ins_qual;
  const int8_t* read_del_qual;
  const int8_t* gcp;
  const int64_t* hap_lengths;  /* [batch], 1..max_hap_len */
  const int64_t* read_lengths; /* [batch], 1..max_read_len */
} gklhip_pdhmm_batch;

/* The reads x haplotypes form of IntelPDHMM.computeLikelihoods (IntelPDHMM.java:83-145): every read against every
 * haplotype, out[r * n_haps + h] (JavaData.h:177-242 builds exactly this cross product as padded PAIRS before calling
 * computePDHMM; here each read and each haplotype crosses PCIe once). */
typedef struct {
  int32_t n_reads, n_haps;
  int32_t max_hap_len;       /* row stride of the two haplotype arrays */
  int32_t max_read_len;      /* row stride of the five read arrays */
  const int8_t* hap_bases;   /* [n_haps][max_hap_len] */
  const int8_t* hap_pdbases;
  const int8_t* read_bases;  /* [n_reads][max_read_len] */
  const int8_t* read_qual;
  const int8_t* read_ins_qual;
  const int8_t* read_del_qual;
  const int8_t* gcp;
  const int64_t* hap_lengths;  /* [n_haps] */
  const int64_t* read_lengths; /* [n_reads] */
} gklhip_pdhmm_cross;

/* With GKL_HIP_SERVER=PATH (non-empty) in the environment this is gklhip_pdhmm_connect(PATH, device, out_ctx): the
 * process makes no HIP call. */
int gklhip_pdhmm_init(int device /* -1 = current */, gklhip_pdhmm_ctx** out_ctx);

/* ---- client mode: the context's calls are computed by the server on socket_path (gkl_amd/lib/gklhip_server,
 * INTEGRATION.md section 6), which loads libgklhip_pdhmm.so and keeps one context of its own per client context.  The
 * client process makes no HIP call.  Every function of this header works on a client context: set_fma_mode /
 * set_tail_mode are kept here and travel with every call (GKL_HIP_PDHMM_TAIL is read by the client at init, as
 * always), the compute calls check their arguments here first, with the same statuses and messages, last_kernel_ms /
 * last_routing return what the server's context reported for the call, buffer_bytes is the size of the shared-memory
 * arena.  GKL_HIP_PDHMM_TABLE and GKL_HIP_PDHMM_PIPELINE belong to the process that computes: the server.
 * device: -1 = the server's choice (its --devices list, else its current device). */
int gklhip_pdhmm_connect(const char* socket_path, int device, gklhip_pdhmm_ctx** out_ctx);
int gklhip_pdhmm_is_remote(gklhip_pdhmm_ctx* ctx);
/* The server's PDHMM counters (its PairHMM ones: gklhip_server_stats of gkl_hip_pairhmm.h).  Fixed size. */
typedef struct {
  int32_t protocol, pid;
  int32_t library_state;     /* 0: no client has asked for PDHMM yet, 1: libgklhip_pdhmm.so loaded, -1: loading failed */
  int32_t reserved0;
  int64_t calls_served, calls_failed;
  int32_t calls_active;
  int32_t live_connections;  /* PDHMM connections = PDHMM contexts the server holds */
  int64_t connections_total;
  int64_t pairs_served;      /* pairs of the calls that succeeded */
  int64_t combine_counts[3]; /* gklhip_pdhmm_combine_counts of the server process, summed over its devices */
  int64_t reserved[6];
} gklhip_pdhmm_server_info;
int gklhip_pdhmm_server_stats(const char* socket_path, gklhip_pdhmm_server_info* out);

/* 1 (default) = bit-identical to GKL's AVX-512 PDHMM object (avx512_impl.cc: a*b + c*d contracted to
 * fma(c, d, a*b)); 0 = bit-identical to its AVX2 object (avx2_impl.cc: no FMA).  Same switch as
 * gklhip_config.fma_mode of the PairHMM. */
int gklhip_pdhmm_set_fma_mode(gklhip_pdhmm_ctx* ctx, int fma_mode);
/* GKL finishes the last `batch mod SIMD width` pairs of every vector batch with its scalar engine (pdhmm.h:1264-1270 ->
 * pdhmm-serial.cc:279-412), whose arithmetic differs from its vector kernels': a pair's value depends on its position
 * in the batch.  mode 1 ("reference", the DEFAULT; GKL_HIP_PDHMM_TAIL=reference): the pairs at positions
 * >= batch - batch mod W (W = 8 with fma_mode 1 = the AVX-512 engine, 4 with fma_mode 0 = AVX2) of a paired batch -- and
 * of every reference batch of a cross product, see gklhip_pdhmm_compute_cross_batched -- take the scalar engine's
 * arithmetic, so that EVERY position matches GKL bit for bit.  mode 0 ("vector"; GKL_HIP_PDHMM_TAIL=vector in the
 * environment at init): the vector arithmetic for every pair -- position-independent results. */
int gklhip_pdhmm_set_tail_mode(gklhip_pdhmm_ctx* ctx, int mode);
/* Host buffers in, out_host[batch] = log10 likelihoods. Negative ins/del/gcp quals ->
 * GKLHIP_ERR_INVALID_ARG (PDHMM_INPUT_DATA_ERROR in the reference). */
int gklhip_pdhmm_compute(gklhip_pdhmm_ctx* ctx, const gklhip_pdhmm_batch* batch, double* out_host);
/* out_host[n_reads * n_haps], read-major. Same arithmetic, errors and tables as gklhip_pdhmm_compute; in tail mode 1 the
 * whole cross product counts as ONE reference batch (= gklhip_pdhmm_compute_cross_batched with ref_batch_pairs 0). */
int gklhip_pdhmm_compute_cross(gklhip_pdhmm_ctx* ctx, const gklhip_pdhmm_cross* batch, double* out_host);
/* The reference's computeLikelihoodsNative cuts the read-major pair list into batches of
 * min(total, maxMemoryInMB / memoryPerPair) pairs (pdhmm/JavaData.h:83-101) and every batch ends in its own scalar tail.
 * ref_batch_pairs replays that cut in tail mode 1 (0: one batch); gklhip_pdhmm_reference_batch_pairs computes the
 * reference's number from the memory limit and the two maximum lengths.  The limit is what initNative kept:
 * gklhip_pdhmm_available_memory_mb(maxMemoryInMB) = min(maxMemoryInMB, the host's free RAM), taken once at
 * initialisation like the reference's getMaxMemoryAvailable (pdhmm-implementation.h:204-235), so that identical calls
 * are cut -- and therefore rounded -- identically.  What the JNI shim's computeLikelihoodsNative calls. */
int gklhip_pdhmm_compute_cross_batched(gklhip_pdhmm_ctx* ctx, const gklhip_pdhmm_cross* batch, int64_t ref_batch_pairs, double* out_host);
/* ---- device-resident calls: the byte arrays and the results stay in HBM (cf. gklhip_compute_device of the PairHMM) ----
 * dev_batch: the seven byte arrays (hap_bases, hap_pdbases, read_bases, read_qual, read_ins_qual, read_del_qual, gcp) are
 * addresses in HBM on the context's device, same row strides as in the host calls; hap_lengths and read_lengths are HOST
 * arrays as always (the planner and the argument checks read them).  out_dev: [n_pairs] doubles in HBM, in the host
 * call's order (paired: by position; cross: r * n_haps + h).  sums_dev: NULL, or [n_pairs] doubles in HBM that receive
 * the raw sums of the same pairs -- bit for bit the doubles the host calls finalise.
 * Ordering: the library's work is ordered behind everything already enqueued on hip_stream (a hipStream_t; NULL = HIP's
 * default stream): an event recorded there, which the context's stream waits for.  The calls are SYNCHRONOUS: they return
 * after the context's stream has drained, the results are in place and the status is final.  There is no asynchronous
 * variant.  The cross call waits once early as well: its planner reads haplotype bytes on the host, so hap_bases and
 * hap_pdbases (n_haps * max_hap_len bytes each) are first copied back to pinned host memory, behind the caller's
 * stream; the read arrays -- the bulk -- never leave the device.
 * Arithmetic: fma mode, tail mode and ref_batch_pairs act exactly as in the host calls, and the sums are the host calls'
 * bit for bit.  out_dev[i] = log10(sum[i]) - log10(2^1020) is evaluated ON THE DEVICE in double: it is NOT guaranteed to
 * be bit-identical to the host calls' output, which takes glibc's log10 like GKL (differences are in the last bits).  A
 * caller that needs GKL's bits asks for sums_dev and finalises them with gklhip_pdhmm_finalise_host.
 * Errors: the argument checks of the host calls, with the same statuses and texts (a NULL out_dev like a NULL out_host),
 * before anything touches the device.  A negative ins / del / gcp quality is found on the device as in the host calls:
 * GKLHIP_ERR_INVALID_ARG, and out_dev and sums_dev are left untouched.  On a client context of the server both return
 * GKLHIP_ERR_UNSUPPORTED before anything else.  These calls never enter the combiner and do not count in
 * gklhip_pdhmm_combine_counts; gklhip_pdhmm_last_routing and gklhip_pdhmm_last_kernel_ms (the forward launches, not the
 * finalisation) report as after the host call of the same problem. */
int gklhip_pdhmm_compute_device(gklhip_pdhmm_ctx* ctx, const gklhip_pdhmm_batch* dev_batch, double* out_dev,
                                double* sums_dev /* may be NULL */, void* hip_stream);
int gklhip_pdhmm_compute_cross_device(gklhip_pdhmm_ctx* ctx, const gklhip_pdhmm_cross* dev_batch, int64_t ref_batch_pairs,
                                      double* out_dev, double* sums_dev /* may be NULL */, void* hip_stream);
/* The host calls' finalisation of n raw sums (host arrays): out[i] = log10(sums[i]) - log10(2^1020) with the host libm.
 * Needs no context and makes no HIP call. */
int gklhip_pdhmm_finalise_host(const double* sums, int64_t n, double* out);
/* Several region calls in ONE set of launches: region k's output is, byte for byte, what
 * gklhip_pdhmm_compute_cross_batched(ctx, &regions[k], ref_batch_pairs[k], out_host[k]) writes on the same context -- whichever
 * other regions ride along, in whatever order, in both fma modes and both tail modes (tail mode 1: every region is cut into
 * its own reference batches with its own scalar tails).  The regions are planned one by one as single calls are; their
 * inputs then cross PCIe in one copy, their job tables in another, and the device runs one entries kernel, at most one
 * launch each of the table, predicate and byte-comparing kernels and one tail launch for all of them; one host
 * finalisation.  ref_batch_pairs: [n_regions], NULL = all 0.  out_host: [n_regions] pointers, region k's n_reads * n_haps
 * doubles.  status_out: [n_regions] or NULL.
 * Returns GKLHIP_OK when every region succeeded, else the status of the first failing region (gklhip_pdhmm_last_error: its
 * message); the per-region statuses are in status_out and the regions that succeeded have valid results.  The argument
 * checks of the single call run per region before anything touches the device: a region that fails them is left out and
 * the rest still run; so does a region with a negative quality (GKLHIP_ERR_INVALID_ARG) -- the others are not affected.  A
 * HIP failure of the shared launches fails every region in them.
 * Limits of a shared launch set: 64 regions, 4 MB of inputs at the common row strides (the largest max_read_len /
 * max_hap_len of the regions), 131 072 pairs in total.  A call over any of them -- and every call on a client context, whose
 * wire protocol has no multi request -- is computed region by region through the single-call path, with the same results.
 * Afterwards gklhip_pdhmm_last_routing holds the sums over the regions and gklhip_pdhmm_last_kernel_ms the time of the
 * shared launches (region by region: the sum of the calls' times). */
int gklhip_pdhmm_compute_cross_multi(gklhip_pdhmm_ctx* ctx, int32_t n_regions, const gklhip_pdhmm_cross* regions,
                                     const int64_t* ref_batch_pairs, double* const* out_host, int32_t* status_out);
/* The two combined: several region calls whose byte arrays already lie in HBM, in ONE set of launches, the results left in
 * HBM region by region.  dev_regions: [n_regions], each as dev_batch of gklhip_pdhmm_compute_cross_device (the seven byte
 * arrays in HBM on the context's device, at the region's own row strides and at any alignment; hap_lengths and read_lengths
 * on the host).  ref_batch_pairs: [n_regions], NULL = all 0.  out_dev: [n_regions] HBM pointers, region k's n_reads * n_haps
 * doubles.  sums_dev: NULL, or [n_regions] HBM pointers of which any may be NULL.  status_out: [n_regions] or NULL.  The
 * pointer arrays themselves are host arrays.
 * Ordering: SYNCHRONOUS, like gklhip_pdhmm_compute_cross_device: the work is ordered behind everything already enqueued
 * on hip_stream (an event recorded there, which the context's stream waits for) and the call returns after the context's
 * stream has drained.  It waits once early: one gather kernel copies all regions' arrays, device to device, to the common
 * row strides of the set, and both haplotype arrays of all regions come back to pinned host memory in one copy for the
 * planner.  There is no asynchronous variant.
 * Results: region k's sums_dev[k] and out_dev[k] are byte for byte what gklhip_pdhmm_compute_cross_device(ctx,
 * &dev_regions[k], ref_batch_pairs[k], ...) writes on the same context -- whichever regions ride along, in whatever order,
 * in both fma modes and both tail modes (both calls evaluate out = log10(sum) - log10(2^1020) through one device
 * function).  The sums are therefore the host calls' bits too, and gklhip_pdhmm_finalise_host of them gives GKL's values.
 * Errors: as gklhip_pdhmm_compute_cross_multi, with the same statuses and texts.  The argument checks of the single call
 * run per region before anything touches the device (a NULL out_dev[k] like a NULL out_host): a region that fails them
 * is left out and the rest run.  A region with a negative ins / del / gcp quality gets GKLHIP_ERR_INVALID_ARG, its
 * out_dev[k] / sums_dev[k] stay untouched and the other regions are not affected.  A HIP failure of the shared launches
 * fails every region in them.  Return value and gklhip_pdhmm_last_error: the first failing region's.  On a client context:
 * GKLHIP_ERR_UNSUPPORTED before anything else.
 * Limits: those of a shared launch set (64 regions, 4 MB of inputs at the common row strides, 131 072 pairs); a call over
 * any of them is computed region by region through gklhip_pdhmm_compute_cross_device's path, with the same results.
 * Counters: unlike the single device-resident calls, which count nothing, this call counts in gklhip_pdhmm_combine_counts
 * exactly as the host multi call does -- a shared set of n regions adds n calls, n shared calls when n > 1, and 1 set;
 * region by region adds (1, 0, 1) per region -- because the counters are the only observable that shows that the regions
 * shared their launches.  gklhip_pdhmm_last_routing holds the sums over the regions, gklhip_pdhmm_last_kernel_ms the
 * forward launches of the set (not the gather, not the finalisation; region by region: the sum of the calls' times).  The
 * call never enters the combiner. */
int gklhip_pdhmm_compute_cross_multi_device(gklhip_pdhmm_ctx* ctx, int32_t n_regions, const gklhip_pdhmm_cross* dev_regions,
                                            const int64_t* ref_batch_pairs, double* const* out_dev,
                                            double* const* sums_dev /* may be NULL */, int32_t* status_out, void* hip_stream);
/* Process-wide counters of the cross calls computed on `device` by contexts of this process (-1: summed over the devices;
 * client contexts compute nothing and count nothing): out[0] region calls computed, out[1] region calls that shared a
 * launch set with another (gklhip_pdhmm_compute_cross_multi with two or more regions in the set; concurrent calls joined
 * by the combiner), out[2] launch sets.  reset != 0 zeroes them.
 * The combiner (off by default): with GKL_HIP_PDHMM_COMBINE=1 in the environment of the process that computes, cross calls
 * that fit the limits above and meet on a device -- the threads of one JVM, the session threads of the server -- leave as
 * one multi call: the first thread that finds the device's combiner free leads, takes every queued call with its own fma
 * and tail mode up to the limits and runs them on its context.  GKL_HIP_PDHMM_COMBINE_MIN=k (default 1) with
 * GKL_HIP_PDHMM_COMBINE_WAIT_US=t (default 0) lets a leader wait up to t microseconds for k calls; the wait is bounded, a
 * leader whose company does not arrive runs with what it has.  Results are the single call's, byte for byte.  The paired
 * entry point (gklhip_pdhmm_compute) is never combined. */
int gklhip_pdhmm_combine_counts(int device, int64_t out[3], int reset);
int32_t gklhip_pdhmm_available_memory_mb(int32_t max_memory_mb);
int64_t gklhip_pdhmm_reference_batch_pairs(int32_t max_memory_mb, int32_t max_read_len, int32_t max_hap_len, int64_t total_pairs);
/* HIP-event time of the forward kernel of the last call, milliseconds. */
float gklhip_pdhmm_last_kernel_ms(gklhip_pdhmm_ctx* ctx);
/* Diagnostics: bytes of device and pinned host memory the context holds right now.  Its buffers grow with the biggest call
 * and are given back when the last 16 calls each needed less than a quarter of a buffer above 32 MB. */
int64_t gklhip_pdhmm_buffer_bytes(gklhip_pdhmm_ctx* ctx);
/* Diagnostics: how the last cross call's haplotypes were routed: out[0] to the table kernel (at most six classes of
 * (base, SNP alleles, 'N') columns: the match priors come from an LDS table), out[1] to the predicate kernel, out[2] to
 * the byte-comparing kernel (a base outside ACGTN).  After a paired call (gklhip_pdhmm_compute; every pair its own haplotype
 * item, classes and routing found on the device): the call's packed jobs -- wavefront-loads of whole pairs -- by kernel in
 * the same order (a job is the table kernel's when all its haplotypes are eligible).  GKL_HIP_PDHMM_TABLE=0 disables the
 * table kernel.  Results are identical whichever kernel computes a pair. */
int gklhip_pdhmm_last_routing(gklhip_pdhmm_ctx* ctx, int32_t out[3]);
int gklhip_pdhmm_done(gklhip_pdhmm_ctx* ctx);
/* host-built tables as uploaded: 0 qualToErrorProb[255], 1 matchToMatchProb[32640] */
int64_t gklhip_pdhmm_get_table(int which, double* dst, int64_t cap);
const char* gklhip_pdhmm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GKL_HIP_PDHMM_H */
