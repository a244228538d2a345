/*
 * zkmi.h — C ABI of the MI355X-native BN254 Groth16 proving backend
 * (libzkmi.so, zelana_amd/csrc/).  Drop-in replacement for the arithmetic that
 * Zelana's `Groth16Prover` delegates to arkworks 0.5.0:
 *
 *   reference call site                                   replaced by
 *   ---------------------------------------------------   --------------------------
 *   core/src/sequencer/settlement/prover.rs:263-277        zkmi_pk_load
 *     ProvingKey::<Bn254>::deserialize_compressed
 *   core/src/sequencer/settlement/prover.rs:408            zkmi_groth16_prove
 *     Groth16::<Bn254>::prove (create_proof_with_reduction)
 *   ark-groth16 LibsnarkReduction::witness_map_from_       zkmi_witness_map
 *     matrices (3P)
 *   ark-poly Radix2EvaluationDomain::{fft,ifft}[_coset]    zkmi_ntt / zkmi_ntt_device
 *     (3P, a6)
 *   ark-ec VariableBaseMSM::msm_bigint on G1 / G2          zkmi_msm_g1 / zkmi_msm_g2
 *     (3P, a7 / a8; called 4x G1 + 1x G2 per proof)        (+ _device variants)
 *   core/src/sequencer/settlement/prover.rs:304-334        zkmi_proof_to_solana_bytes
 *     Groth16Prover::proof_to_solana_bytes
 *   prover/src/snarkjs.rs:44-52 export_proof_json           zkmi_proof_serialize_compressed
 *
 * Conventions:
 *   - every function returns 0 on success, a negative ZKMI_E* code otherwise;
 *     zkmi_last_error() returns a thread-local message.  Nothing unwinds across
 *     the ABI.
 *   - field elements cross as 4 x uint64 little-endian CANONICAL integers
 *     (never Montgomery); scalars must be < r (arkworks into_bigint()).
 *   - G1 affine = x || y (8 u64), G2 affine = x.c0 || x.c1 || y.c0 || y.c1
 *     (16 u64); the point at infinity is all-zero.
 *   - buffers are caller-owned; calls are synchronous; one context per device
 *     (one process per GPU); a context must not be used by two threads at once.
 *   - the library never falls back to the CPU: without a usable gfx950 device
 *     zkmi_ctx_create fails with ZKMI_ENODEV.
 */
#ifndef ZKMI_H
#define ZKMI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZKMI_OK 0
#define ZKMI_EINVAL (-1)   /* bad argument / malformed input */
#define ZKMI_ENODEV (-2)   /* no usable GPU */
#define ZKMI_EHIP (-3)     /* HIP runtime error */
#define ZKMI_ENOMEM (-4)   /* device allocation failed, or a fixed-size device store could overflow
                            * (zkmi_account_tree_apply past max_nodes) */
#define ZKMI_EPOINT (-5)   /* point not on curve / not in subgroup */

typedef struct zkmi_ctx zkmi_ctx;
typedef struct zkmi_bases zkmi_bases;
typedef struct zkmi_pk zkmi_pk;
typedef struct zkmi_msm_job zkmi_msm_job;
typedef struct zkmi_r1cs_dev zkmi_r1cs_dev;

const char* zkmi_last_error(void);
int zkmi_version(void);

/* ------------------------------------------------------------- context */
int zkmi_ctx_create(int device, zkmi_ctx** out);
/* Destroy the objects made on a context (base sets, keys, device R1CS,
 * communicators, MSM jobs) before the context.  Witness programs may outlive
 * it: zkmi_ctx_destroy detaches them, and zkmi_wprog_destroy then only frees
 * their buffers. */
void zkmi_ctx_destroy(zkmi_ctx* ctx);
/* per-kernel timing with HIP events on the context's stream (bench/profiling) */
int zkmi_profile_enable(zkmi_ctx* ctx, int on);
/* total milliseconds and launch count recorded for kernel `name` */
int zkmi_profile_get(zkmi_ctx* ctx, const char* name, double* total_ms, uint64_t* count);
int zkmi_profile_reset(zkmi_ctx* ctx);
/* device memory staging (so callers can keep inputs resident in HBM) */
int zkmi_dev_alloc(zkmi_ctx* ctx, size_t bytes, void** dptr);
int zkmi_dev_free(zkmi_ctx* ctx, void* dptr);
int zkmi_h2d(zkmi_ctx* ctx, void* dst, const void* src, size_t bytes);
int zkmi_d2h(zkmi_ctx* ctx, void* dst, const void* src, size_t bytes);
int zkmi_sync(zkmi_ctx* ctx);

/* ------------------------------------------------------------- MSM */
/* Upload affine bases once (pk queries stay resident in HBM).  Points are
 * validated on-curve; converted to the device's internal Montgomery form. */
int zkmi_bases_create_g1(zkmi_ctx* ctx, const uint64_t* affine, size_t n, zkmi_bases** out);
int zkmi_bases_create_g2(zkmi_ctx* ctx, const uint64_t* affine, size_t n, zkmi_bases** out);
void zkmi_bases_destroy(zkmi_bases* b);
size_t zkmi_bases_len(const zkmi_bases* b);
/* canonical affine copy of a base set (n x 8 or n x 16 u64) */
int zkmi_bases_export(const zkmi_bases* b, uint64_t* affine_out);
/* Fixed-base table for a base set that is reused across MSMs (a proving
 * key's queries).  Stores `factor` shifted copies 2^(c*Wp*j) * P_i (Wp =
 * ceil(W(c)/factor)) in HBM; later MSMs on this set with window c (the
 * default unless zkmi_msm_set_window pins another) run Wp windows of
 * factor*n entries instead of W(c) windows of n entries: same additions,
 * 1/factor of the bucket reduction.  c = 0 picks the window for len(b);
 * factor = 0 means a full table (one window).  Results are unchanged.
 * Memory: factor x the base set.  No counterpart in the reference
 * (arkworks recomputes every window per proof). */
int zkmi_bases_precompute(zkmi_bases* b, int c, int factor);
/* [len, table window c (0 = none), copies, windows per copy] */
int zkmi_bases_info(const zkmi_bases* b, uint64_t out[4]);
/* Deterministic synthetic inputs generated directly in HBM (benchmarks):
 * bases P_i = k_i * G (k_i from a splitmix64 stream of seed), scalars uniform
 * in [0, r) by rejection.  d_scalars must hold n x 32 bytes. */
int zkmi_bases_generate_g1(zkmi_ctx* ctx, uint64_t seed, size_t n, zkmi_bases** out);
int zkmi_bases_generate_g2(zkmi_ctx* ctx, uint64_t seed, size_t n, zkmi_bases** out);
int zkmi_scalars_generate(zkmi_ctx* ctx, uint64_t seed, size_t n, void* d_scalars);
/* The same streams from global element `first` on: element i of the range is
 * element first + i of the unsharded set, so a point-sharded MSM over ranks
 * [r*n, (r+1)*n) sums to the single-GPU result (multi-GPU bench, config 5). */
int zkmi_bases_generate_range_g1(zkmi_ctx* ctx, uint64_t seed, size_t first, size_t n, zkmi_bases** out);
int zkmi_scalars_generate_range(zkmi_ctx* ctx, uint64_t seed, size_t first, size_t n, void* d_scalars);
/* SURVEY.md §8d's point stream: P_i = P0 + (first + i) * D for i < n
 * (canonical affine P0, D; the bench draws them as G1::rand from
 * StdRng::seed_from_u64(1020)), generated in HBM. */
int zkmi_bases_generate_arith_g1(zkmi_ctx* ctx, const uint64_t p0[8], const uint64_t d[8], size_t first, size_t n,
                                 zkmi_bases** out);

/* sum_{i<n} scalars[i] * bases[offset + i]; n <= len - offset.
 * Host scalars (n x 4 u64). Result: canonical affine. */
int zkmi_msm_g1(zkmi_ctx* ctx, const zkmi_bases* b, size_t offset, const uint64_t* scalars, size_t n,
                uint64_t out_affine[8]);
int zkmi_msm_g2(zkmi_ctx* ctx, const zkmi_bases* b, size_t offset, const uint64_t* scalars, size_t n,
                uint64_t out_affine[16]);
/* same with scalars already resident in device memory (n x 32 B) */
int zkmi_msm_g1_device(zkmi_ctx* ctx, const zkmi_bases* b, size_t offset, const void* d_scalars, size_t n,
                       uint64_t out_affine[8]);
int zkmi_msm_g2_device(zkmi_ctx* ctx, const zkmi_bases* b, size_t offset, const void* d_scalars, size_t n,
                       uint64_t out_affine[16]);
/* Asynchronous form: submit queues the GPU work (and the copy of the ~c*W
 * window bit-sums) on the context stream and returns at once; wait finishes
 * the O(windows) host epilogue and frees the job.  Submitting MSM k+1 before
 * waiting on MSM k overlaps k's epilogue with k+1's kernels.  Scalars must
 * stay valid until wait returns. */
int zkmi_msm_submit(zkmi_ctx* ctx, const zkmi_bases* b, size_t offset, const void* d_scalars, size_t n,
                    zkmi_msm_job** job);
int zkmi_msm_wait(zkmi_msm_job* job, uint64_t* out_affine);
/* window size override for experiments (0 = automatic) */
/* k MSMs with the same device scalars and range over k base sets (e.g. a,
 * b_g1 and b_g2 queries of a proving key, all weighted by z): one digits +
 * sort pass is shared by every set with the same window plan.  jobs[i] is the
 * job of bs[i] (finish each with zkmi_msm_wait). */
int zkmi_msm_submit_shared(zkmi_ctx* ctx, const zkmi_bases* const* bs, int k, size_t offset, const void* d_scalars,
                           size_t n, zkmi_msm_job** jobs);
int zkmi_msm_set_window(zkmi_ctx* ctx, int c);
/* nb MSMs over ONE base set and range: vector i = n scalars at d_scalars +
 * i * stride bytes (stride >= n * 32, a multiple of 32).  The vectors are
 * split into groups (zkmi_ctx_set_batch_group); a group runs as one launch
 * sequence whose sort keys carry the batch index as an outer window, so the
 * short dependent kernels of a small MSM carry a group's work.  Results equal
 * nb zkmi_msm_submit calls.  One job; finish it with zkmi_msm_batch_wait
 * (zkmi_msm_wait on it, zkmi_msm_batch_wait on a single job, or another nb
 * return ZKMI_EINVAL and leave the job valid).  nb = 0 and n = 0 are valid.
 * Batch jobs take no communicator.  No counterpart in the reference. */
int zkmi_msm_batch_submit(zkmi_ctx* ctx, const zkmi_bases* b, size_t offset, const void* d_scalars, size_t n,
                          size_t nb, size_t stride, zkmi_msm_job** job);
/* out = nb canonical affine points (nb x 8 or nb x 16 u64) */
int zkmi_msm_batch_wait(zkmi_msm_job* job, uint64_t* out, size_t nb);
/* proofs / MSMs per batched launch sequence: 0 = automatic (by size), 1..64 */
int zkmi_ctx_set_batch_group(zkmi_ctx* ctx, int g);
int zkmi_ctx_get_batch_group(const zkmi_ctx* ctx);
/* Number of MSM lanes (streams with their own scratch) used round-robin by
 * consecutive submissions so their latency-bound tails overlap; 1..8, at most
 * 2 while a communicator exists on the context (stream budget, below). */
int zkmi_msm_set_lanes(zkmi_ctx* ctx, int lanes);
/* lanes in effect (after the communicator cap) */
int zkmi_msm_get_lanes(const zkmi_ctx* ctx);
/* streams the library holds for this context (context stream, MSM lanes,
 * communicator and witness-program streams) */
int zkmi_ctx_stream_count(const zkmi_ctx* ctx);

/* canonical affine point arithmetic helpers (host) */
int zkmi_g1_add(const uint64_t a[8], const uint64_t b[8], uint64_t out[8]);
int zkmi_g2_add(const uint64_t a[16], const uint64_t b[16], uint64_t out[16]);

/* ------------------------------------------------------------- multi-GPU
 * MSM point sharding (BASELINE.json configs[4]): one rank per
 * GPU (one process per GPU, or one host thread per GPU in one process), each
 * holding its own zkmi_ctx and the shard [first, first + count) of the bases
 * resident in its HBM (zkmi_shard_range + zkmi_bases_create_*).  A sharded MSM
 * runs the full Pippenger pipeline on every shard, then exchanges the
 * per-window bit sums (the partially reduced buckets, ~c x W XYZZ points per
 * rank) with ONE all-gather and sums them across ranks in the group-law
 * epilogue: the "all-reduce of partial bucket sums" (RCCL has no elliptic-
 * curve reduction operator).  Every rank returns the global sum.
 *
 * Transports:
 *   zkmi_comm_init       RCCL (ncclAllGather over xGMI), enqueued on the MSM
 *                        lane's stream: no host round trip in the exchange.
 *                        The ranks' unique id comes from zkmi_comm_unique_id
 *                        on one rank, broadcast by the host (like NCCL).
 *   zkmi_comm_init_host  the host supplies the all-gather (MPI, a TCP store,
 *                        pipes ...): for hosts without RCCL, or ranks that share
 *                        one GPU (RCCL refuses two ranks on one device).
 * Collectives must be issued in the same order on every rank.  Every sharded
 * MSM is exactly one all-gather of one fixed size per rank (a status block and
 * the bit sums), whatever each rank's shard, plan or local failure, so no rank
 * can block in a collective its peers skip.  Ranks' window plans must agree
 * (equal shard sizes and the same zkmi_bases_precompute / zkmi_msm_set_window
 * choice); a mismatch, or a failure on any rank, is reported as ZKMI_EINVAL
 * on every rank by zkmi_msm_wait.
 * Streams: a process with a communicator uses the context stream, at most two
 * MSM lanes (zkmi_msm_set_lanes is capped at 2 while a communicator exists)
 * and the communicator's stream: 4 = GPU_MAX_HW_QUEUES, so the RCCL kernel,
 * which waits for its peers, never shares a hardware queue with a lane's
 * kernels.  Witness programs run on the context stream then. */
typedef struct zkmi_comm zkmi_comm;
#define ZKMI_COMM_ID_BYTES 128
/* all-gather of `bytes` from every rank: recv = rank 0's bytes || rank 1's ... */
typedef int (*zkmi_allgather_fn)(void* user, const void* send, void* recv, size_t bytes);
int zkmi_comm_unique_id(uint8_t id[ZKMI_COMM_ID_BYTES]);
int zkmi_comm_init(zkmi_ctx* ctx, const uint8_t id[ZKMI_COMM_ID_BYTES], int nranks, int rank, zkmi_comm** out);
int zkmi_comm_init_host(zkmi_ctx* ctx, int nranks, int rank, zkmi_allgather_fn allgather, void* user,
                        zkmi_comm** out);
void zkmi_comm_destroy(zkmi_comm* comm);
/* [nranks, rank, transport (0 = RCCL, 1 = host)] */
int zkmi_comm_info(const zkmi_comm* comm, int out[3]);
/* contiguous point shard of rank `rank`: the first total % nranks ranks get
 * one extra point */
int zkmi_shard_range(size_t total, int nranks, int rank, size_t* first, size_t* count);
/* sum over ALL ranks of sum_{i<n} scalars[i] * shard[offset + i]; collective.
 * Scalars are this rank's slice (device memory, n x 32 B canonical).  A
 * rank-local failure fails the MSM on every rank.  Over RCCL it is returned by
 * the submit; over a host transport the submit returns a job and
 * zkmi_msm_wait returns the error, because that transport's exchanges run in
 * wait order (the failure joins the exchange of its own job, never an earlier
 * job's still in flight). */
int zkmi_msm_sharded_submit(zkmi_comm* comm, const zkmi_bases* shard, size_t offset, const void* d_scalars,
                            size_t n, zkmi_msm_job** job);
int zkmi_msm_sharded(zkmi_comm* comm, const zkmi_bases* shard, size_t offset, const void* d_scalars, size_t n,
                     uint64_t* out_affine);
/* Window sharding (north_star's "Pippenger windows sharded across GPUs"):
 * every rank passes the WHOLE base set and scalars (n points, resident on its
 * GPU) and runs windows [r W / N, (r + 1) W / N) of the plain Pippenger plan
 * (window c = zkmi_msm_set_window, 12..17 bits, or 0 for the automatic
 * choice, clamped to 12..17; a fixed-base table is not used -- it folds
 * every window into one).  The same
 * fixed-size exchange as the point-sharded MSM hands each rank's window bit
 * sums to every rank, and zkmi_msm_wait assembles all W windows (each from
 * the one rank that ran it) before the Horner epilogue: every rank returns
 * the whole MSM.  Collective, like zkmi_msm_sharded_submit.  Replaces the
 * same call site (prover.rs:408 via ark-ec msm_bigint). */
int zkmi_msm_window_sharded_submit(zkmi_comm* comm, const zkmi_bases* bases, size_t offset, const void* d_scalars,
                                   size_t n, zkmi_msm_job** job);

/* ------------------------------------------------------------- NTT */
/* In-place radix-2 transform over Fr of length 2^log_n, natural order in and
 * out, ark-poly semantics: inverse=0 -> evaluations at omega^k (times g^i
 * coefficient scaling when coset=1, g = 5); inverse=1 -> interpolation incl.
 * n^-1 (and g^-i when coset=1).  log_n <= 28. */
int zkmi_ntt(zkmi_ctx* ctx, uint64_t* data, uint32_t log_n, int inverse, int coset);
int zkmi_ntt_device(zkmi_ctx* ctx, void* d_data, uint32_t log_n, int inverse, int coset);
/* nb transforms in one launch sequence: vector i at d_data + i * stride bytes
 * (stride >= 2^log_n * 32, a multiple of 32; nb <= 65535).  Bytes between two
 * vectors are not written. */
int zkmi_ntt_batch_device(zkmi_ctx* ctx, void* d_data, uint32_t log_n, size_t nb, size_t stride, int inverse,
                          int coset);

/* ------------------------------------------------------------- Groth16 */
/* R1CS in CSR form; variable 0 = One, instance i -> i, witness j ->
 * num_instance + j (ark-relations to_matrices).  Coefficients canonical Fr. */
typedef struct {
  size_t num_constraints, num_instance, num_witness;
  const uint64_t* a_rowptr; const uint64_t* a_col; const uint64_t* a_val;
  const uint64_t* b_rowptr; const uint64_t* b_col; const uint64_t* b_val;
  const uint64_t* c_rowptr; const uint64_t* c_col; const uint64_t* c_val;
} zkmi_r1cs;

/* witness map: h (2^ceil(log2(m + l)) canonical Fr), natural order */
int zkmi_witness_map(zkmi_ctx* ctx, const zkmi_r1cs* cs, const uint64_t* z, uint64_t* h_out);

/* Load an arkworks-serialized ProvingKey<Bn254> (compressed=1 as read by
 * Groth16Prover::from_bytes, or uncompressed=0).  Points are decompressed /
 * validated on the GPU and stay resident. */
int zkmi_pk_load(zkmi_ctx* ctx, const uint8_t* bytes, size_t len, int compressed, zkmi_pk** out);
void zkmi_pk_destroy(zkmi_pk* pk);
/* [n_domain, num_instance, num_witness] */
int zkmi_pk_info(const zkmi_pk* pk, uint64_t out[3]);
/* arkworks-compressed VerifyingKey bytes embedded in the pk (for vk hash) */
/* Fixed-base tables for all five queries (zkmi_bases_precompute, window
 * picked per query length; factor 0 = full).  Proofs are unchanged; a full
 * table costs ~15x the key's HBM footprint (2^22 domain: ~24 GB).  When at
 * least 1/8 of the variables have both B bases at infinity (B_i(t) = 0: no B
 * row reads them), the B-query MSMs are first compacted to the others. */
int zkmi_pk_precompute(zkmi_pk* pk, int factor);
/* number of variables the B-query MSMs run over (V - 1 when not compacted) */
int zkmi_pk_b_terms(const zkmi_pk* pk, uint64_t* out);
int zkmi_pk_vk_bytes(const zkmi_pk* pk, uint8_t* buf, size_t cap, size_t* len);

/* Full proof.  z: full assignment (One, instance..., witness...), canonical.
 * r, s: the blinding scalars (the caller draws them from StdRng::seed_from_u64
 * (batch_id) in arkworks order r then s, as Groth16::prove does).
 * Outputs: canonical affine A (G1), B (G2), C (G1). */
int zkmi_groth16_prove(zkmi_ctx* ctx, const zkmi_pk* pk, const zkmi_r1cs* cs, const uint64_t* z,
                       const uint64_t r[4], const uint64_t s[4], uint64_t a_out[8], uint64_t b_out[16],
                       uint64_t c_out[8]);

/* Circuit matrices resident in HBM: a proving key fits exactly one circuit
 * shape (keygen.rs proves dummy()'s shape), so the
 * matrices are uploaded once and only the witness changes per proof. */
int zkmi_r1cs_create(zkmi_ctx* ctx, const zkmi_r1cs* cs, zkmi_r1cs_dev** out);
void zkmi_r1cs_destroy(zkmi_r1cs_dev* cs);
/* prove with R1CS and assignment z (n_vars x 32 B canonical) already in HBM */
int zkmi_groth16_prove_resident(zkmi_ctx* ctx, const zkmi_pk* pk, const zkmi_r1cs_dev* cs, const void* d_z,
                                const uint64_t r[4], const uint64_t s[4], uint64_t a_out[8], uint64_t b_out[16],
                                uint64_t c_out[8]);
/* Asynchronous form of the resident prove: submit queues the witness map and
 * the five MSMs and returns; wait finishes the MSM epilogues and the
 * assembly.  Several proofs may be in flight on one context (finish them in
 * submission order); d_z must stay unchanged until its proof's wait returns,
 * unless a zkmi_wprog_run writing it is ordered after (see there). */
typedef struct zkmi_proof_job zkmi_proof_job;
int zkmi_groth16_prove_submit(zkmi_ctx* ctx, const zkmi_pk* pk, const zkmi_r1cs_dev* cs, const void* d_z,
                              const uint64_t r[4], const uint64_t s[4], zkmi_proof_job** job);
int zkmi_groth16_prove_wait(zkmi_proof_job* job, uint64_t a_out[8], uint64_t b_out[16], uint64_t c_out[8]);
/* nb proofs of same-shape witnesses under one key: assignment i at d_z + i *
 * z_stride bytes (the layout zkmi_wprog_run_many writes; z_stride >= n_vars *
 * 32, a multiple of 32), blinding scalars r[4 i ..], s[4 i ..].  Domains up to
 * 2^16: groups of proofs (zkmi_ctx_set_batch_group) run as ONE launch
 * sequence each -- a batched witness map and batched MSMs -- instead of ~130
 * launches per proof; larger domains run the single-proof schedule with two
 * proofs in flight.  Proofs equal zkmi_groth16_prove_resident's, byte for
 * byte.  d_z stays unchanged until wait returns; jobs of a context are
 * finished in submission order (single and batched alike).  The reference
 * proves such a stream one Groth16::prove at a time (prover.rs:408). */
int zkmi_groth16_prove_many_submit(zkmi_ctx* ctx, const zkmi_pk* pk, const zkmi_r1cs_dev* cs, const void* d_z,
                                   size_t nb, size_t z_stride, const uint64_t* r, const uint64_t* s,
                                   zkmi_proof_job** job);
/* a_out nb x 8, b_out nb x 16, c_out nb x 8; nb must equal the job's */
int zkmi_groth16_prove_many_wait(zkmi_proof_job* job, size_t nb, uint64_t* a_out, uint64_t* b_out, uint64_t* c_out);
int zkmi_groth16_prove_many(zkmi_ctx* ctx, const zkmi_pk* pk, const zkmi_r1cs_dev* cs, const void* d_z, size_t nb,
                            size_t z_stride, const uint64_t* r, const uint64_t* s, uint64_t* a_out, uint64_t* b_out,
                            uint64_t* c_out);
/* R1CS satisfaction of assignments resident in HBM (arkworks
 * ConstraintSystem::is_satisfied / which_is_unsatisfied; the reference proves
 * in release mode, where nothing checks the witness).  What is checked are
 * the rows: <a_i,z> <b_i,z> = <c_i,z> mod r for every i < num_constraints.
 * z[0] = 1 and z < r remain the caller's contract. */
#define ZKMI_ROW_NONE UINT64_MAX
typedef struct {
  uint64_t first_row;          /* lowest i with <a_i,z><b_i,z> != <c_i,z>; ZKMI_ROW_NONE if every row holds */
  uint64_t n_bad;              /* number of such rows */
  uint64_t a[4], b[4], c[4];   /* canonical <a_i,z>, <b_i,z>, <c_i,z> at first_row; zero if none */
} zkmi_r1cs_status;
/* nb assignments (z_i at d_z + i * z_stride, the prove_many layout: z_stride
 * >= n_vars * 32, a multiple of 32) against a resident R1CS; synchronous.
 * Runs the witness map's mat-vecs (no transform) in chunks of assignments
 * (zkmi_ctx_set_batch_group, or automatic: a bounded workspace) and one scan
 * over their outputs.  out: nb statuses; nb = 0 is valid. */
int zkmi_r1cs_check(zkmi_ctx* ctx, const zkmi_r1cs_dev* cs, const void* d_z, size_t nb, size_t z_stride,
                    zkmi_r1cs_status* out);
/* Proof jobs submitted while on also check their witness: the scan runs on
 * the witness map's mat-vec outputs, before the transforms overwrite them.
 * Off by default; off, no kernel or copy is added.  Proofs are the same bytes
 * either way, and a wait returns the proof and ZKMI_OK whether or not the
 * witness is satisfied (the reference's semantics): the status is
 * information, not an error.  A job keeps the setting it was submitted
 * with. */
int zkmi_ctx_set_prove_check(zkmi_ctx* ctx, int on);
int zkmi_ctx_get_prove_check(const zkmi_ctx* ctx);
/* statuses of the proofs of the proof job most recently WAITED on this
 * context, in proof order; *count = 0 if that job was submitted with the
 * check off; ZKMI_EINVAL if cap < count (*count is still set) */
int zkmi_groth16_last_check(zkmi_ctx* ctx, zkmi_r1cs_status* out, size_t cap, size_t* count);
/* Benchmark helper: a random proving key of domain 2^log_n with the given
 * instance/witness counts, generated in HBM.  Proofs made with it do not
 * verify; the proving work is identical to a real key of that shape. */
int zkmi_pk_synthetic(zkmi_ctx* ctx, uint64_t seed, uint32_t log_n, size_t num_instance, size_t num_witness,
                      zkmi_pk** out);

/* Groth16 circuit-specific setup on the GPU.  Replaces
 * Groth16::<Bn254>::circuit_specific_setup (prover/src/bin/keygen.rs:87-91,
 * ark-groth16 0.5 generate_parameters_with_qap): QAP evaluation at t over the
 * radix-2 domain, then every query point as a fixed-base multiple of the
 * generators.  The caller draws the randomness in arkworks' order from its
 * StdRng (alpha, beta, gamma, delta = Fr::rand; G1::rand; G2::rand; then
 * t = Fr::rand until t^n != 1):
 *   toxic = alpha | beta | gamma | delta | t   (5 x 4 u64, canonical Fr)
 *   g1 (8 u64), g2 (16 u64)                     canonical affine generators
 * The key is resident (as after zkmi_pk_load) and equals arkworks' key for
 * the same inputs. */
int zkmi_groth16_setup(zkmi_ctx* ctx, const zkmi_r1cs* cs, const uint64_t toxic[20], const uint64_t g1[8],
                       const uint64_t g2[16], zkmi_pk** out);
/* VerifyingKey::deserialize_compressed (points decoded and validated on the
 * GPU) then serialize_compressed: the bytes Groth16Prover::compute_vk_hash
 * hashes (core/src/sequencer/settlement/prover.rs:266-267, 289-294).
 * out = NULL queries the length. */
int zkmi_vk_canonical(zkmi_ctx* ctx, const uint8_t* bytes, size_t len, uint8_t* out, size_t cap, size_t* out_len);
/* ProvingKey::serialize_compressed of a resident key (keygen.rs:101-104);
 * buf = NULL queries the length. */
int zkmi_pk_serialize(const zkmi_pk* pk, uint8_t* buf, size_t cap, size_t* len);

/* ------------------------------------------------------------- encodings */
/* 256 B Solana layout: -A (x,y LE) || B (x.c0,x.c1,y.c0,y.c1 LE) || C (x,y LE)
 * (prover.rs:304-334) */
int zkmi_proof_to_solana_bytes(const uint64_t a[8], const uint64_t b[16], const uint64_t c[8],
                               uint8_t out[256]);
/* 128 B arkworks Proof::serialize_compressed (a 32 || b 64 || c 32) */
int zkmi_proof_serialize_compressed(const uint64_t a[8], const uint64_t b[16], const uint64_t c[8],
                                    uint8_t out[128]);

/* ------------------------------------------------------ witness programs
 * Per-batch witness generation on the GPU: a proving
 * key fits one circuit shape, so a batch's full assignment z is a fixed
 * straight-line program over Fr of its ~thousands of free inputs (for
 * zelana_batch: Prover.toml's values; 99% of z is MiMC round values,
 * prover-worker/src/mimc.rs:52-142).  The program is recorded once on the
 * host (zelana_amd/wprog.py); per batch only the inputs travel, and z is
 * written straight into HBM for zkmi_groth16_prove_resident.
 *   op i: 4 x u32 {kind | a_len << 8 | b_len << 20, out, a_off, b_off};
 *         kinds 1 MUL z[out] = <a,z><b,z>; 2 INV z[out] = <a,z>^-1 (0 -> 0);
 *         3 BITS64 z[out+i] = bit i of <a,z>; 4 PERM MiMC permutation of
 *         <a,z>: z[out + 4r + (0..3)] = t_r^2, t_r^4, t_r^6, t_r^7 (91 rounds,
 *         t_0 = <a,z> + c_0, t_r = t_{r-1}^7 + c_r, c_i = (i+1)^3 + (i+1))
 *         5 BITS z[out+i] = bit i of <a,z>, i < b_off (1..256; b_len = 0);
 *         6 NZ z[out] = (<a,z> != 0); 8 INV1 z[out] = <a,z>^-1, or 1 when it
 *         is 0 (r1cs-std is_neq's two witnesses);
 *         7 POSEIDON one permutation of L2BlockCircuit's width-3 Poseidon
 *         sponge (prover/src/l2_circuit.rs:68-83: x^5, 8 full + 56 partial
 *         rounds).  State in: three combinations stored back to back at
 *         a_off, of lengths a_len, b_len and b_off & 0xFFFF; mask = b_off >> 16
 *         (1..7) marks the elements that are variables in round 0.  Out: x^2,
 *         x^4, x^5 of every S-box in round order (round 0 only for masked
 *         elements): 3 popcount(mask) + 231 values.  Reads the round
 *         constants ark[r][i] at coefficient 3r + i and the MDS matrix
 *         m[i][j] at 192 + 3i + j (so num_coeffs >= 201);
 *         9 POSEIDON_RC kind 7's op with the round counts in the op (for
 *         ShieldedTransferCircuit's sponge, prover/src/circuit/shielded.rs:
 *         365-368: 8 full + 57 partial rounds).  b_off holds: bits 0-15 the
 *         third combination's length, bits 16-18 the mask (1..7), bits 19-26
 *         R_p, bits 27-31 R_f / 2 (>= 1; R_f + R_p <= 72).  Combinations,
 *         quad mapping and trace order as kind 7; out: 3 popcount(mask) +
 *         9 (R_f/2 - 1) + 3 R_p + 9 R_f/2 values (3 popcount(mask) + 234 for
 *         8 + 57).  Reads ark[r][i] at coefficient 3r + i and m[i][j] at
 *         3 (R_f + R_p) + 3i + j (so num_coeffs >= 3 (R_f + R_p) + 9).  Every
 *         kind-9 op of a program has the same R_f and R_p, and a program
 *         holds kind 7 or kind 9 ops, not both (either table starts at
 *         coefficient 0);
 *         10 SELECT z[out] = <c,z> != 0 ? <t,z> : <f,z> (r1cs-std
 *         AllocatedFp::conditionally_select's witness): c, t, f stored back to
 *         back at a_off, of lengths a_len, b_len and b_off & 0xFFFF (b_off's
 *         upper bits 0).
 *         Of a kind 7 / 9 trace only the last round's three x^5 may be read
 *         by other ops, of a kind 4 trace only the permutation's output, the
 *         last round's t^7 (the rest stays in Montgomery form until the run's
 *         last kernels); zkmi_wprog_create refuses a term that reads another
 *         trace value (ZKMI_EINVAL).
 *   term: 2 x u32 {z index, coefficient index}; <a,z> = sum over
 *         term[a_off .. a_off + a_len) of coeff * z
 *   levels: ops [level_start[l], level_start[l+1]) depend only on inputs and
 *         earlier levels.  A level may hold any mix of kinds in ANY order
 *         (and may be empty): how it is launched is decided from all its ops,
 *         so z is the same for every order; recorders put permutations first
 *         only so that the quads of a wave share a kind.  A level is one
 *         launch, except runs of small levels (<= 256 ops each) with no
 *         permutation (kinds 4, 7, 9) or SELECT in them, and runs of small
 *         levels made of kinds 9 and 10 alone, which one workgroup steps
 *         through in one launch (ZKMI_DEBUG_WPROG_NO_RC_CHAIN=1 in the environment
 *         of zkmi_wprog_create turns the second kind of run off: a
 *         measurement switch). */
typedef struct zkmi_wprog zkmi_wprog;
typedef struct {
  size_t num_vars;                             /* |z| */
  size_t num_inputs; const uint32_t* input_var; /* z index of input k */
  size_t num_ops; const uint32_t* op;           /* num_ops x 4 */
  size_t num_terms; const uint32_t* term;       /* num_terms x 2 */
  size_t num_coeffs; const uint64_t* coeff;     /* num_coeffs x 4, canonical Fr */
  size_t num_levels; const uint32_t* level_start; /* num_levels + 1 */
} zkmi_wprog_desc;
int zkmi_wprog_create(zkmi_ctx* ctx, const zkmi_wprog_desc* desc, zkmi_wprog** out);
void zkmi_wprog_destroy(zkmi_wprog* prog);
/* z (device, num_vars x 32 B) <- the program over `inputs` (num_inputs x 4
 * u64 canonical; input 0 is One = 1).  Later work on the context (a proof
 * over z) waits for it.  async = 1: returns after queueing on the program's
 * own stream, which runs beside the context's earlier work (the previous
 * proof); it then waits only for context work queued before the PREVIOUS
 * run, so callers alternate two z buffers. */
int zkmi_wprog_run(zkmi_ctx* ctx, zkmi_wprog* prog, const uint64_t* inputs, void* d_z, int async);
/* nb batches in one run (one launch sequence; the kernels are latency-bound,
 * so nb batches take about the time of one): inputs = nb x num_inputs x 4
 * u64, batch i's z at d_z + i * z_stride bytes (z_stride >= num_vars * 32, a
 * multiple of 32).  Same ordering rules as zkmi_wprog_run, with buffer sets in
 * place of buffers. */
int zkmi_wprog_run_many(zkmi_ctx* ctx, zkmi_wprog* prog, size_t nb, const uint64_t* inputs, void* d_z,
                        size_t z_stride, int async);

/* ------------------------------------------------- verification / on-chain
 * Host code (no GPU needed).  The reference's Groth16Prover::verify is a
 * length check (prover.rs:427-442); the real check is the on-chain verifier's
 * (onchain-programs/verifier/programs/onchain_verifier/src/lib.rs:497-547),
 * restated here so a host can check its proofs before settling them. */
/* ark-groth16 verify_proof: vk = arkworks-compressed VerifyingKey bytes (as
 * Groth16Prover::from_bytes reads them; decoded and validated, G2 subgroup
 * included); inputs = n canonical Fr (4 x u64), n = IC count - 1.
 * *valid = 1 iff e(A,B) = e(alpha,beta) e(IC[0] + sum x_i IC[i+1], gamma) e(C,delta). */
int zkmi_groth16_verify(const uint8_t* vk, size_t vk_len, const uint64_t* inputs, size_t n_inputs,
                        const uint64_t a[8], const uint64_t b[16], const uint64_t c[8], int* valid);
/* The alt_bn128 syscalls the on-chain verifier calls (EIP-196/197 big-endian:
 * G1 = x || y, G2 = x.c1 || x.c0 || y.c1 || y.c0, (0,0) = infinity; points
 * validated, G2 in the order-r subgroup).  pairing: k x 192 bytes -> 32-byte
 * big-endian 1 iff prod e(P_i, Q_i) = 1. */
int zkmi_alt_bn128_pairing(const uint8_t* input, size_t len, uint8_t out[32]);
int zkmi_alt_bn128_g1_add(const uint8_t in[128], uint8_t out[64]);
int zkmi_alt_bn128_g1_mul(const uint8_t in[96], uint8_t out[64]);
/* The 256-B proof in the syscalls' big-endian encoding: -A || B || C
 * (the big-endian flag of proof_to_solana_bytes, whose reference output is
 * little-endian: SURVEY.md App. B.3). */
int zkmi_proof_to_alt_bn128_bytes(const uint64_t a[8], const uint64_t b[16], const uint64_t c[8], uint8_t out[256]);
/* batch_inputs_to_field_elements (verifier lib.rs:479-494): the six 32-byte
 * roots as given, then batch_id as a 32-byte big-endian field element */
int zkmi_batch_inputs_alt_bn128(const uint8_t roots[6 * 32], uint64_t batch_id, uint8_t out[7 * 32]);
/* k * P on G1 (canonical affine): ProverNode::generate_fragment's single scalar
 * multiplication (forge/prover/src/lib.rs:351-358); with zkmi_g1_add it covers
 * the forge's <= 7-point Lagrange sums (:252-290) */
int zkmi_g1_mul(const uint64_t p[8], const uint64_t k[4], uint64_t out[8]);

/* ------------------------------------------------- batched verification
 * zkmi_groth16_verify for nb proofs under one key, with the Miller loops on
 * the GPU.  With weights rho_i (non-zero, 128 bits)
 *   prod_i e(rho_i A_i, B_i) e(-(sum rho_i) alpha, beta)
 *     e(-sum rho_i X_i, gamma) e(-sum rho_i C_i, delta) = 1
 * is nb + 3 Miller loops (one GPU lane each, two kernels on the context
 * stream: no new stream) and ONE final exponentiation on the host.  If it
 * holds, every proof that passed point validation is valid.  If not, the host
 * bisects over the per-proof Miller values: a probe is a subset product, the
 * subset's three fixed pairs and one final exponentiation, at most two probes
 * a level; a subset of one is decided exactly.  A valid proof is never
 * rejected; an invalid one is accepted with probability about 2^-127 over the
 * weights.  Worst case without a probe budget: every proof bad costs about
 * 2 nb probes, slower than a loop of zkmi_groth16_verify.  With a budget B
 * (zkmi_ctx_set_verify_probes) the host runs at most B final exponentiations
 * and the proofs still undecided then get exact verdicts from ONE pass of
 * zkmi_groth16_verify_each's kernels, whose cost does not depend on how many
 * proofs are bad. */
typedef struct zkmi_vk zkmi_vk;
/* arkworks-compressed VerifyingKey, decoded and validated once (as
 * zkmi_groth16_verify does per call); ZKMI_EPOINT for a bad key */
int zkmi_vk_load(zkmi_ctx* ctx, const uint8_t* bytes, size_t len, zkmi_vk** out);
void zkmi_vk_destroy(zkmi_vk* vk); /* before the context, like keys and base sets */
int zkmi_vk_info(const zkmi_vk* vk, uint64_t out[1]); /* [n_inputs] */
/* pairs: Miller loops run on the GPU (nb + 3); final_exps: host final
 * exponentiations (1 when every proof is valid); invalid_points: proofs that
 * failed point validation */
typedef struct {
  uint64_t pairs;
  uint64_t final_exps;
  uint64_t invalid_points;
} zkmi_verify_stats;
/* valid[i] = what zkmi_groth16_verify returns for proof i (up to the
 * soundness error above).  inputs: nb x n_inputs x 4 u64, each < r (else
 * ZKMI_EINVAL for the whole call); a bad proof point is valid[i] = 0, not an
 * error.  nb = 0 is valid and launches nothing.  Synchronous.
 * rho: NULL = the library draws the weights from the OS (getrandom) inside
 * the call, after the proofs are fixed -- the only sound use: a prover who
 * knows the weights before choosing its proofs can make invalid proofs cancel
 * in the combined check.  Non-NULL rho (nb x 2 u64, each 128-bit value
 * non-zero, else ZKMI_EINVAL) exists for reproducible tests only. */
int zkmi_groth16_verify_many(zkmi_ctx* ctx, const zkmi_vk* vk, size_t nb, const uint64_t* inputs, const uint64_t* a,
                             const uint64_t* b, const uint64_t* c, const uint64_t* rho, uint8_t* valid,
                             zkmi_verify_stats* stats);

/* ------------------------------------------------- per-proof verification
 * zkmi_groth16_verify for nb proofs under one key with EVERYTHING on the GPU
 * (DESIGN.md section 2.8): per proof the three Miller loops of (A_i, B_i),
 * (-X_i, gamma), (-C_i, delta), one more for (-alpha, beta) per call, and one
 * final exponentiation per proof, a GPU lane each.  valid[i] equals
 * zkmi_groth16_verify's verdict for proof i exactly: there are no weights and
 * no soundness error, and the cost is the same whether the proofs are valid or
 * not (a fixed number of launches on the context stream, no new stream).  Only
 * the nb verdict bytes (and the validation flags) come back to the host.
 * pairs: Miller loops run (3 nb + 1, or 0 when no proof passed point
 * validation); final_exps: GPU final exponentiations (the proofs that passed
 * point validation); invalid_points: as in zkmi_verify_stats. */
typedef struct {
  uint64_t pairs;
  uint64_t final_exps;
  uint64_t invalid_points;
} zkmi_verify_each_stats;
/* The argument rules of zkmi_groth16_verify_many: an input >= r is
 * ZKMI_EINVAL for the whole call, a bad proof point is valid[i] = 0, nb = 0
 * is valid and launches nothing, a key of another context is ZKMI_EINVAL.
 * Synchronous. */
int zkmi_groth16_verify_each(zkmi_ctx* ctx, const zkmi_vk* vk, size_t nb, const uint64_t* inputs, const uint64_t* a,
                             const uint64_t* b, const uint64_t* c, uint8_t* valid, zkmi_verify_each_stats* stats);
/* Probe budget of zkmi_groth16_verify_many on this context.  0 (the default):
 * unlimited, nothing changes.  B >= 1: host final exponentiations are counted,
 * the first combined check included; once B have run, every proof not yet
 * decided goes in one sub-batch through zkmi_groth16_verify_each's kernels
 * (over the points already uploaded and validated), so stats.final_exps <= B
 * and the call's cost is bounded however many proofs are bad.
 * Recommended where bad batches can occur: 20.  Measured (DESIGN.md section
 * 2.8) a probe costs about 6.3 ms of host time and the hand-over about 121 ms
 * whatever nb is, so the two cost the same at about 19 probes: one bad proof
 * among up to 1024 (at most 1 + 2 log2 nb = 21 probes, 20 measured) is still
 * found by bisection, two or more are handed over.  The default stays 0. */
int zkmi_ctx_set_verify_probes(zkmi_ctx* ctx, uint64_t max_probes);
uint64_t zkmi_ctx_get_verify_probes(const zkmi_ctx* ctx);
/* What the last zkmi_groth16_verify_many on this context handed to the GPU
 * when its budget ran out: out = {gpu_decided (proofs), gpu_pairs (Miller
 * loops of that sub-batch), gpu_final_exps}; all 0 when the budget was not
 * hit. */
int zkmi_groth16_verify_last(zkmi_ctx* ctx, uint64_t out[3]);

/* ------------------------------------------------- proofs from wire bytes
 * The inverses of the proof encoders, and the batched verifiers over encoded
 * proofs, decoded on the GPU (which has the decoding
 * rule as a table).  A decoder tells two failures apart:
 *   malformed      wrong length, unknown format, a coordinate >= q, a flag the
 *                  format does not allow, a compressed x with no root
 *   invalid point  a well-formed encoding of a point off the curve / twist, or
 *                  of a B outside the order-r subgroup (the checks of
 *                  zkmi_groth16_verify)
 * Compressed: x < q after masking the two flag bits; bit 6 of the last byte =
 * infinity and then every other bit, bit 7 included, is zero; otherwise y is
 * the root selected by bit 7 (y > -y; Fq2 compares c1 first).  Every accepted
 * 128-byte string re-serializes to itself.  Uncompressed: every coordinate
 * < q after masking the point's last byte; bit 6 as above; bit 7 ignored; y
 * as given.  SOLANA_LE / ALT_BN128_BE: no flag bits, every coordinate < q,
 * all-zero = infinity, A's y comes back as q - y when y != 0: the exact
 * inverses of the two encoders. */
#define ZKMI_PROOF_ARK_COMPRESSED   0  /* 128 B: A32 | B64 | C32, SWFlags (zkmi_proof_serialize_compressed) */
#define ZKMI_PROOF_ARK_UNCOMPRESSED 1  /* 256 B: A64 | B128 | C64, flags in each point's last byte */
#define ZKMI_PROOF_SOLANA_LE        2  /* 256 B: -A | B | C little-endian, no flags (zkmi_proof_to_solana_bytes) */
#define ZKMI_PROOF_ALT_BN128_BE     3  /* 256 B: -A | B | C big-endian, G2 as c1|c0 (zkmi_proof_to_alt_bn128_bytes) */
size_t zkmi_proof_encoded_len(int fmt); /* 0 for an unknown fmt */
/* One proof, on the host (no context).  0 and canonical affine points, or
 * ZKMI_EINVAL (malformed) / ZKMI_EPOINT (invalid point) with a, b, c zeroed. */
int zkmi_proof_decode(int fmt, const uint8_t* in, size_t len, uint64_t a[8], uint64_t b[16], uint64_t c[8]);
/* nb proofs back to back (nb x zkmi_proof_encoded_len(fmt) bytes), decoded
 * and validated on the GPU (context stream).  a / b / c: nb x 8 / 16 / 8 u64;
 * status[i]: 0 ok, 1 malformed, 2 invalid point; the rows of a non-ok proof
 * are zero.  Equals zkmi_proof_decode proof by proof. */
int zkmi_proofs_decode(zkmi_ctx* ctx, int fmt, const uint8_t* proofs, size_t nb, uint64_t* a, uint64_t* b,
                       uint64_t* c, uint8_t* status);
/* zkmi_groth16_verify_many / _each over encoded proofs: the bytes are
 * uploaded as they are and decoded by a kernel into the buffers the verify
 * kernels read.  valid[i] is zkmi_groth16_verify's verdict on
 * zkmi_proof_decode's points, 0 when that decode fails; malformed (nb bytes
 * or NULL) is 1 for the proofs whose encoding is malformed, and those count in
 * stats.invalid_points.  All argument rules of the point-taking calls hold
 * (inputs >= r, nb = 0, a key of another context, rho, the probe budget and
 * zkmi_groth16_verify_last); an unknown fmt is ZKMI_EINVAL. */
int zkmi_groth16_verify_many_encoded(zkmi_ctx* ctx, const zkmi_vk* vk, int fmt, size_t nb, const uint8_t* proofs,
                                     const uint64_t* inputs, const uint64_t* rho, uint8_t* valid, uint8_t* malformed,
                                     zkmi_verify_stats* stats);
int zkmi_groth16_verify_each_encoded(zkmi_ctx* ctx, const zkmi_vk* vk, int fmt, size_t nb, const uint8_t* proofs,
                                     const uint64_t* inputs, uint8_t* valid, uint8_t* malformed,
                                     zkmi_verify_each_stats* stats);

/* ----------------------------------- Poseidon hashing / note commitment tree
 * The Poseidon sponge over Fr as a primitive (width 3: rate 2, capacity 1,
 * x^5), one GPU lane per hash, and an append-only Merkle tree over it that
 * lives in device memory.  Field elements are 4 x
 * u64 little-endian.  Every INPUT may be any 256-bit value and is taken mod r
 * (Fr::from_le_bytes_mod_order); every output is canonical.  All calls run on
 * the context stream, return with their results on the host and open no
 * stream (zkmi_ctx_stream_count is unchanged).  Destroy hashers and trees
 * before their context, and a tree before its hasher. */
typedef struct zkmi_poseidon zkmi_poseidon;     /* resident constants of one parameter set */
/* consts: (3 (R_f + R_p) + 9) x 4 words in the order of a kind-9 op's table:
 * ark[r][i] at 3 r + i, then mds[i][j].  ZKMI_EINVAL unless full_rounds is
 * even and >= 2 and full_rounds + partial_rounds <= 72. */
int zkmi_poseidon_create(zkmi_ctx* ctx, uint32_t full_rounds, uint32_t partial_rounds, const uint64_t* consts,
                         zkmi_poseidon** out);
void zkmi_poseidon_destroy(zkmi_poseidon* ph);
/* out[i] = absorb(in[i * arity .. i * arity + arity)); squeeze one element.
 * arity 1..4 (else ZKMI_EINVAL); in: n x arity x 4, out: n x 4 words, host
 * pointers; n = 0 does nothing. */
int zkmi_poseidon_hash_many(zkmi_ctx* ctx, const zkmi_poseidon* ph, size_t n, uint32_t arity, const uint64_t* in,
                            uint64_t* out);

/* The tree of the reference's MerkleTree: leaves at level 0, parent = H(left,
 * right), a node with no leaf below it reads as e_level, where e_0 =
 * empty_leaf and e_{l+1} = H(e_l, e_l); the root of an empty tree is e_depth.
 * Level l stores ceil(capacity / 2^l) nodes of 32 bytes (64 MB for 2^20
 * leaves).  depth 1..32, capacity 1..2^depth leaves, else ZKMI_EINVAL. */
typedef struct zkmi_note_tree zkmi_note_tree;
int zkmi_note_tree_create(zkmi_ctx* ctx, const zkmi_poseidon* ph, uint32_t depth, uint64_t capacity,
                          const uint64_t empty_leaf[4], zkmi_note_tree** out);
void zkmi_note_tree_destroy(zkmi_note_tree* t);
int zkmi_note_tree_info(const zkmi_note_tree* t, uint64_t out[3]); /* depth, capacity, next_position */
/* The n leaves go to positions [next, next + n) and every node above them is
 * rehashed once.  *first (may be NULL) = the old next_position.  roots (may
 * be NULL): n x 4 words, roots[k] = the root after leaf k alone of this call
 * has been added to everything before it (what n single insertions would have
 * returned one by one).  An append past the capacity is ZKMI_EINVAL and leaves
 * the tree, its root and next_position as they were; n = 0 does nothing. */
int zkmi_note_tree_append(zkmi_ctx* ctx, zkmi_note_tree* t, size_t n, const uint64_t* leaves, uint64_t* first,
                          uint64_t* roots);
int zkmi_note_tree_root(zkmi_ctx* ctx, const zkmi_note_tree* t, uint64_t out[4]);
/* siblings: n x depth x 4 words, the leaf level first; the is-right bit of
 * level l is bit l of the position.  A position >= next_position fails the
 * whole call with ZKMI_EINVAL and nothing is written. */
int zkmi_note_tree_paths(zkmi_ctx* ctx, const zkmi_note_tree* t, size_t n, const uint64_t* positions,
                         uint64_t* siblings);
/* out: the leaves [first, first + n) as stored (canonical); ZKMI_EINVAL when
 * the range passes next_position */
int zkmi_note_tree_leaves(zkmi_ctx* ctx, const zkmi_note_tree* t, uint64_t first, size_t n, uint64_t* out);

/* ------------------------------------------------ MiMC hashing / account tree
 * The MiMC sponge of the zelana_batch circuit as a primitive (91 rounds of
 * x <- (x + c_i)^7, c_i = (i+1)^3 + (i+1), key 0; hash_k(x_1..x_k) = the
 * sponge over [k, x_1, .., x_k]), one GPU lane per hash, and the sparse
 * account tree over it with batched ORDERED leaf writes (DESIGN.md section
 * 2.12).  Field elements are 4 x u64 little-endian.  Every INPUT may be any
 * 256-bit value and is taken mod r; every output is canonical.  All calls run
 * on the context stream, return with their results on the host and open no
 * stream (zkmi_ctx_stream_count is unchanged).  Destroy hashers and trees
 * before their context, and a tree before its hasher. */
typedef struct zkmi_mimc zkmi_mimc;             /* resident round constants and the four P(k) */
int zkmi_mimc_create(zkmi_ctx* ctx, zkmi_mimc** out);
void zkmi_mimc_destroy(zkmi_mimc* mh);
/* out[i] = hash_arity(in[i * arity .. i * arity + arity)).  arity 1..4 (else
 * ZKMI_EINVAL); in: n x arity x 4, out: n x 4 words, host pointers; n = 0
 * does nothing. */
int zkmi_mimc_hash_many(zkmi_ctx* ctx, const zkmi_mimc* mh, size_t n, uint32_t arity, const uint64_t* in,
                        uint64_t* out);

/* The tree of the reference's AccountTree: `depth` levels (1..32) over
 * hash_2, a leaf at any position in [0, 2^depth), a node with no written leaf
 * below it reads as e_level, where e_0 = 0 and e_{l+1} = hash_2(e_l, e_l); the
 * root of an empty tree is e_depth.  Nodes live in an open-addressing table in
 * device memory of max_nodes slots (8 + 32 bytes each), fixed at create: it
 * neither grows nor rehashes.  The table may fill to its last slot, and the
 * cost of that is the caller's: probing is linear, a lookup of an ABSENT node
 * (most siblings of a depth-32 path) walks to the next empty slot, so about
 * 1 / (1 - load)^2 / 2 slots on average and all max_nodes slots once the table
 * is full; apply, paths and leaves then cost O(lookups x max_nodes).  Size
 * max_nodes at twice the nodes expected (load <= 1/2: under 3 slots a lookup).
 * depth outside 1..32 or max_nodes = 0 is ZKMI_EINVAL; ZKMI_ENOMEM when the
 * table cannot be allocated. */
typedef struct zkmi_account_tree zkmi_account_tree;
int zkmi_account_tree_create(zkmi_ctx* ctx, const zkmi_mimc* mh, uint32_t depth, uint64_t max_nodes,
                             zkmi_account_tree** out);
void zkmi_account_tree_destroy(zkmi_account_tree* t);
int zkmi_account_tree_info(const zkmi_account_tree* t, uint64_t out[3]); /* depth, max_nodes, nodes stored */
/* n ordered leaf writes, leaves[k] to positions[k] for k = 0 .. n-1 in this
 * order (a position may repeat), with what n single writes would have seen
 * one by one.  Each output may be NULL:
 *   siblings   n x depth x 4 words: the path of positions[k] as write k sees
 *              it (after the writes before it), the leaf level first; the
 *              is-right bit of level l is bit l of the position;
 *   old_leaves n x 4 words: the leaf that write k replaces (0 when none);
 *   roots      n x 4 words: the root after write k.
 * n <= 65536 and every position < 2^depth, else ZKMI_EINVAL.  A call that
 * could store more than max_nodes nodes, counted as nodes stored + n (depth +
 * 1), is refused with ZKMI_ENOMEM before anything is launched.  A refused
 * call (ZKMI_EINVAL, ZKMI_ENOMEM) leaves the tree, its root and its node count
 * as they were.  The table is written by the call's last launch only, so a
 * call that fails with ZKMI_EHIP before that launch does too; ZKMI_EHIP from
 * the last launch on (a failed copy of the results) may leave the writes
 * applied in the table while the outputs are incomplete: destroy such a tree.
 * n = 0 does nothing. */
int zkmi_account_tree_apply(zkmi_ctx* ctx, zkmi_account_tree* t, size_t n, const uint64_t* positions,
                            const uint64_t* leaves, uint64_t* siblings, uint64_t* old_leaves, uint64_t* roots);
int zkmi_account_tree_root(zkmi_ctx* ctx, const zkmi_account_tree* t, uint64_t out[4]);
/* siblings: n x depth x 4 words against the current state, laid out as
 * above; a position never written returns the e_l.  A position >= 2^depth
 * fails the whole call with ZKMI_EINVAL and nothing is written. */
int zkmi_account_tree_paths(zkmi_ctx* ctx, const zkmi_account_tree* t, size_t n, const uint64_t* positions,
                            uint64_t* siblings);
/* out: n x 4 words, the leaf at positions[i] (0 when never written); a
 * position >= 2^depth is ZKMI_EINVAL with nothing written */
int zkmi_account_tree_leaves(zkmi_ctx* ctx, const zkmi_account_tree* t, size_t n, const uint64_t* positions,
                             uint64_t* out);

/* -------------------------------------------------------------- nullifier set
 * The spent-nullifier set of the shielded pool, resident in device memory,
 * with an ORDERED batched spend.  A key is 32 raw
 * bytes, compared bytewise: unlike every field-element input above it is NOT
 * taken mod r (the reference keeps a HashSet<[u8; 32]>), so a caller whose
 * keys are field elements must refuse non-canonical encodings itself
 * (ShieldedPool.settle does).  The set holds an append-only log of its keys in
 * insertion order (capacity x 32 bytes) and an open-addressing table of
 * `slots` u32 entries, slots = the least power of two >= 2 capacity, fixed at
 * create; nothing is ever removed.  All calls run on the context stream,
 * return with their results on the host and open no stream.  Destroy a set
 * before its context. */
typedef struct zkmi_nullifier_set zkmi_nullifier_set;
#define ZKMI_NF_ACCEPTED      0 /* every key of the transfer is now spent */
#define ZKMI_NF_SKIPPED       1 /* eligible[t] = 0: the transfer took no part */
#define ZKMI_NF_SPENT_STORED  2 /* detail = k: key k was in the set before the call */
#define ZKMI_NF_SPENT_IN_CALL 3 /* detail = u: an accepted earlier transfer u of this call spent the key */
#define ZKMI_NF_DUP_IN_TX     4 /* detail = k: key k equals an earlier key of the same transfer */
/* capacity 0 or above 2^31 is ZKMI_EINVAL; ZKMI_ENOMEM when the log and the
 * table cannot be allocated. */
int zkmi_nullifier_set_create(zkmi_ctx* ctx, uint64_t capacity, zkmi_nullifier_set** out);
void zkmi_nullifier_set_destroy(zkmi_nullifier_set* set);
int zkmi_nullifier_set_info(const zkmi_nullifier_set* set, uint64_t out[3]); /* capacity, slots, keys stored */
/* out[i] = 1 when keys[i] (n x 32 bytes, host) is stored, else 0.  n <= 2^24;
 * n = 0 does nothing. */
int zkmi_nullifier_set_contains(zkmi_ctx* ctx, const zkmi_nullifier_set* set, size_t n, const uint8_t* keys,
                                uint8_t* out);
/* ntx transfers of per_tx keys each (keys: ntx x per_tx x 32 bytes), with the
 * result of taking them one by one, in order:
 *   for t = 0 .. ntx-1:
 *     eligible[t] = 0:                 (SKIPPED, 0); its keys enter nothing
 *     else for k = 0 .. per_tx-1, the first k that fails decides:
 *       key stored before this call:                         (SPENT_STORED, k)
 *       key spent by an ACCEPTED earlier transfer u < t:     (SPENT_IN_CALL, u)
 *       key equal to an earlier key of t:                    (DUP_IN_TX, k)
 *     no k fails: (ACCEPTED, 0), and all keys of t are spent from here on.
 * A refused transfer spends nothing, so a later transfer that shares a key
 * with it alone is accepted.  verdict[t], detail[t]: ntx words each; eligible:
 * ntx bytes, or NULL = all eligible; *rounds (may be NULL) = the parallel
 * rounds the call took (0 when no eligible transfer reached them, 1 or 2 for
 * honest input, the length of the longest chain of transfers each refused or
 * accepted only through the one before it otherwise).  The accepted keys are
 * appended to the log in transfer order, then key order.
 * per_tx outside 1..4 or more than 2^24 keys in a call is ZKMI_EINVAL.  When
 * the accepted keys do not fit the capacity the call returns ZKMI_ENOMEM
 * before anything of the set is written: count, log and contains answers are
 * as before, and verdict / detail are not written.  ZKMI_EHIP from the insert
 * on may leave keys entered while the outputs are incomplete: destroy such a
 * set.  ntx = 0 does nothing. */
int zkmi_nullifier_set_spend(zkmi_ctx* ctx, zkmi_nullifier_set* set, size_t ntx, uint32_t per_tx, const uint8_t* keys,
                             const uint8_t* eligible, uint32_t* verdict, uint32_t* detail, uint32_t* rounds);
/* out: the keys [first, first + n) of the log, n x 32 bytes, in insertion
 * order (what a restart feeds back through spend with per_tx = 1); ZKMI_EINVAL
 * when the range passes the number of keys stored; n = 0 does nothing. */
int zkmi_nullifier_set_log(zkmi_ctx* ctx, const zkmi_nullifier_set* set, uint64_t first, size_t n, uint8_t* out);

/* ------------------------------------------------------- encrypted-note store
 * The encrypted notes of the shielded pool, resident in device memory beside
 * their commitments and positions, and a batched scan that answers "which of
 * these notes are mine" for up to 64 keys in one call (DESIGN.md section
 * 2.14).  A note is what the reference's EncryptedNote holds: an ephemeral
 * X25519 public key (32 bytes), a nonce (12 bytes) and a ChaCha20-Poly1305
 * ciphertext with its 16-byte tag last, over value u64 | randomness 32 |
 * memo_len u16 | memo.  The scan derives, per (key, note) pair, key =
 * BLAKE3 derive_key("zelana-note-v1", X25519(decryption_key, ephemeral_pk) ||
 * ephemeral_pk), checks the tag, decrypts, parses and confirms the commitment.
 * X25519 is RFC 7748 with no contributory check: a low-order ephemeral_pk
 * gives the all-zero shared secret and the scan carries on, as the
 * reference's x25519-dalek does.  The store is append-only and fixed at
 * create: headers in arrays of their own, ciphertexts at a fixed stride of
 * max_ct rounded up to 16 bytes.  All calls run on the context stream, return
 * with their results on the host and open no stream (zkmi_ctx_stream_count is
 * unchanged).  Destroy a store before its context. */
typedef struct zkmi_note_store zkmi_note_store;
#define ZKMI_SCAN_NOT_MINE         0 /* the tag does not match, or the ciphertext is shorter than a tag */
#define ZKMI_SCAN_MALFORMED        1 /* tag good; plaintext under 42 bytes or memo_len past its end */
#define ZKMI_SCAN_WRONG_COMMITMENT 2 /* tag and parse good; the scheme's commitment differs from the stored one */
#define ZKMI_SCAN_HIT              3
#define ZKMI_COMMIT_NONE     0 /* no commitment check (the reference's decrypt_note) */
#define ZKMI_COMMIT_MIMC     1 /* MiMC hash_3(owner_pk, value, randomness): the scan_notes handler */
#define ZKMI_COMMIT_POSEIDON 2 /* the Poseidon sponge over (value, randomness, owner_pk): ShieldedPool's tree */
/* capacity 1..2^26 notes; max_ct 58..65593: the longest ciphertext accepted,
 * tag included (570 covers the reference's 512-byte memo cap).  Else
 * ZKMI_EINVAL; ZKMI_ENOMEM when the arrays (capacity x (88 + max_ct rounded
 * up to 16) bytes) cannot be allocated. */
int zkmi_note_store_create(zkmi_ctx* ctx, uint64_t capacity, uint32_t max_ct, zkmi_note_store** out);
void zkmi_note_store_destroy(zkmi_note_store* store);
int zkmi_note_store_info(const zkmi_note_store* store, uint64_t out[4]); /* capacity, max_ct, notes stored, ciphertext bytes stored */
/* n notes, appended in this order.  positions: n words, in any order, not
 * contiguous; commitments, ephemeral_pks: n x 32 bytes; nonces: n x 12 bytes;
 * ct_lens: n words, each 0..max_ct (a ciphertext too short to open is stored
 * and scans as NOT_MINE); cts: the ciphertexts back to back.  ZKMI_EINVAL for
 * a ct_len above max_ct or a position that repeats one of this call or one
 * stored by an earlier call (a position names one leaf of the commitment
 * tree: two notes there cannot both be right); ZKMI_ENOMEM when the notes do
 * not fit the capacity.  A refused call writes nothing: info, get and scan
 * answer as before.  n = 0 does nothing. */
int zkmi_note_store_append(zkmi_ctx* ctx, zkmi_note_store* store, size_t n, const uint32_t* positions,
                           const uint8_t* commitments, const uint8_t* ephemeral_pks, const uint8_t* nonces,
                           const uint32_t* ct_lens, const uint8_t* cts);
/* The notes [first, first + n) in append order, into the same arrays (what
 * persistence and a restart need); each output may be NULL.  cts receives the
 * ciphertexts back to back: n x max_ct bytes always suffice, and a first call
 * for ct_lens alone gives the exact size.  ZKMI_EINVAL when the range passes
 * the notes stored; n = 0 does nothing. */
int zkmi_note_store_get(zkmi_ctx* ctx, const zkmi_note_store* store, uint64_t first, size_t n, uint32_t* positions,
                        uint8_t* commitments, uint8_t* ephemeral_pks, uint8_t* nonces, uint32_t* ct_lens,
                        uint8_t* cts);
/* Scan every stored note at a position >= from_position with each of nkeys
 * (decryption key, owner public key) pairs (nkeys x 32 bytes each; nkeys <= 64,
 * 0 does nothing), one GPU lane per (key, note) pair.  scheme: ZKMI_COMMIT_*;
 * mh may be NULL unless scheme is MIMC, ph unless it is POSEIDON, else
 * ZKMI_EINVAL.  The commitment's inputs are taken mod r and its canonical
 * little-endian bytes are compared with the stored 32 bytes.  Per key k:
 *   stats[4 k + result]   the pairs of each ZKMI_SCAN_* result over all notes examined;
 *   counts[k]             the hits returned, at most limit (1..65536);
 *   slot k limit + j, j < counts[k], of positions (words), values (u64),
 *   randomness and commitments (32 bytes), memo_lens (words) and memos
 *   (max_ct - 58 bytes a slot; may be NULL): hit j of key k, in ASCENDING
 *   POSITION order; the other slots are not written.  Bytes after a declared
 *   memo are dropped, as the reference drops them;
 *   scanned_to[k]         when more than limit hits exist: the position of the
 *                         last hit returned, so a scan from scanned_to + 1
 *                         loses nothing; otherwise the highest stored position
 *                         >= from_position, or from_position when there is none.
 * (The reference cuts its loop at limit in database-key order and sorts
 * afterwards: a cut answer there is an arbitrary subset.)  The call keeps
 * nkeys x notes x 37 bytes of workspace on the context. */
int zkmi_note_scan(zkmi_ctx* ctx, const zkmi_note_store* store, const zkmi_mimc* mh, const zkmi_poseidon* ph,
                   uint32_t scheme, size_t nkeys, const uint8_t* decryption_keys, const uint8_t* owner_pks,
                   uint32_t from_position, uint32_t limit, uint32_t* counts, uint32_t* scanned_to, uint32_t* stats,
                   uint32_t* positions, uint64_t* values, uint8_t* randomness, uint8_t* commitments,
                   uint32_t* memo_lens, uint8_t* memos);

/* ------------------------------------------------------ Ed25519 verification
 * The signatures of the sequencer's transparent path (transfers and
 * withdrawals), verified in batches, one GPU lane per signature (DESIGN.md
 * section 2.16).  The semantics are ed25519-dalek 2.2.0 `verify` (not
 * verify_strict) over curve25519-dalek 4.1.3, which the reference calls:
 *   - the public key A decompresses by dalek's rules: bit 255 is the sign of
 *     x, the low 255 bits are y and need not be below p (they are reduced),
 *     x = 0 with the sign bit set is accepted; only a y on no point fails;
 *   - s >= L is refused;
 *   - k = SHA-512(R || A as given || M) mod L, and the canonical 32 bytes of
 *     [s]B + [k](-A) are compared with R: no cofactor, a small-order A is
 *     accepted, and a non-canonical R fails because its bytes differ.
 * When several reasons apply, BAD_PUBKEY comes before BAD_S: the reference
 * parses the key first.  The time of a call does not depend on the verdicts. */
#define ZKMI_SIG_OK          0
#define ZKMI_SIG_BAD_PUBKEY  1  /* A does not decompress */
#define ZKMI_SIG_BAD_S       2  /* s >= L */
#define ZKMI_SIG_MISMATCH    3  /* the equation does not hold (a non-canonical R included) */
/* pubkeys: n x 32 bytes; sigs: n x 64 bytes (R, then s); msgs: the messages
 * back to back, of any lengths, 0 included; msg_offsets: n + 1 ascending byte
 * offsets into msgs, [0] = 0, message i = [msg_offsets[i], msg_offsets[i + 1]);
 * verdicts: n bytes, a ZKMI_SIG_* each.  n = 0 does nothing and launches
 * nothing.  ZKMI_EINVAL for a null argument, msg_offsets[0] != 0, offsets that
 * descend, or more than 2^26 signatures; verdicts is then not written.  The
 * call keeps 137 bytes a signature plus the message bytes of workspace on the
 * context (keys, signatures, offsets, k, verdicts), and 2560 bytes a signature
 * for the tables of -A of at most 2^18 signatures at a time (640 MiB at most),
 * beside 2560 bytes for the table of B, made on the context's first call. */
int zkmi_ed25519_verify_many(zkmi_ctx* ctx, size_t n, const uint8_t* pubkeys, const uint8_t* sigs, const uint8_t* msgs,
                             const uint64_t* msg_offsets, uint8_t* verdicts);

/* ------------------------------------------------- Transaction authorisation
 * The whole check the reference's sequencer makes of a transfer or withdrawal
 * before it touches an account (tx_router.rs:668-793), from the transaction's
 * fields: the signed message is built on the device,
 * the human-readable format first and the legacy binary one for those the
 * first did not verify, and `from` is compared with the signer.  The messages
 * are tx_router.rs:624-666 byte for byte; the legacy ones are
 * from || to || amount || nonce || chain_id (88 bytes) and
 * from || to_l1 || amount || nonce (80 bytes) with little-endian integers,
 * which for a transfer ASSUMES wincode's layout as DESIGN.md section 2.16
 * states.  The signature semantics are those of zkmi_ed25519_verify_many. */
#define ZKMI_TX_TRANSFER    0
#define ZKMI_TX_WITHDRAWAL  1
typedef struct {            /* 192 bytes, no implicit padding */
  uint8_t  from[32];
  uint8_t  to[32];          /* a transfer's `to`, a withdrawal's to_l1_address */
  uint64_t amount, nonce, chain_id;   /* chain_id ignored for a withdrawal */
  uint8_t  signer_pubkey[32];
  uint8_t  signature[64];
  uint8_t  kind;            /* ZKMI_TX_* */
  uint8_t  reserved[7];     /* must be zero */
} zkmi_signed_tx;
#ifdef __cplusplus
static_assert(sizeof(zkmi_signed_tx) == 192, "zkmi_signed_tx is 192 bytes");
#else
_Static_assert(sizeof(zkmi_signed_tx) == 192, "zkmi_signed_tx is 192 bytes");
#endif

#define ZKMI_TXAUTH_OK             0
#define ZKMI_TXAUTH_BAD_PUBKEY     1   /* signer_pubkey does not decompress */
#define ZKMI_TXAUTH_FAILED         2   /* neither format verifies (s >= L included) */
#define ZKMI_TXAUTH_FROM_MISMATCH  3   /* a format verified and from != signer_pubkey */
#define ZKMI_TXFMT_NONE 0
#define ZKMI_TXFMT_READABLE 1
#define ZKMI_TXFMT_LEGACY 2
/* txs: n records, transfers and withdrawals in any mix; reasons: n bytes, a
 * ZKMI_TXAUTH_* each; formats: n bytes, the ZKMI_TXFMT_* that verified (NONE
 * unless the reason is OK or FROM_MISMATCH).  In the order of the reference's
 * bail!s: the key is judged first; the readable format is tried; the legacy
 * format is tried only for records whose readable check gave
 * ZKMI_SIG_MISMATCH (an s >= L fails under both and is not tried again); `from`
 * is compared with the signer only when a format verified.  n = 0 does nothing
 * and launches nothing.  ZKMI_EINVAL for a null argument, a kind that is no
 * ZKMI_TX_*, a reserved byte that is not zero, or more than 2^26 records;
 * neither output is then written.  The call keeps 540 bytes a record of
 * workspace on the context (the record 192, its message slot 304, the length,
 * k, the retry list, two verdicts, reason and format), and shares
 * zkmi_ed25519_verify_many's tables: 2560 bytes a record for at most 2^18
 * records at a time, and the table of B. */
int zkmi_tx_auth_many(zkmi_ctx* ctx, size_t n, const zkmi_signed_tx* txs, uint8_t* reasons, uint8_t* formats);

#ifdef __cplusplus
}
#endif
#endif
