/*
 * zigz_hip.h -- C ABI of libzigz_hip.so: the MI355X (gfx950) backend for zigz's data-parallel
 * hot path (BabyBear MLE bind/eval, sumcheck rounds, SHA3 Merkle commit/open, Lasso fingerprints).
 *
 * This is the drop-in boundary.  The reference (Zig, single-threaded, no FFI of its own) keeps its
 * host code; each entry point below replaces the body of ONE reference function, cited per
 * declaration as reference file:line.  A Zig `extern "c"` shim that binds these symbols is shown
 * in INTEGRATION.md.
 *
 * Conventions (mirroring the reference):
 *  - Field elements cross the boundary as canonical u64 little-endian values in [0, p),
 *    p = 2013265921 (BabyBear, src/core/field_presets.zig:19) -- the in-memory layout of
 *    `[]F` for `F = Field(u64, p)` (src/core/field.zig:27), so Zig slices pass as-is.
 *    Non-canonical inputs are rejected with ZIGZ_ERR_NOT_CANONICAL.
 *  - Results are written into caller-allocated buffers (Zig callers own every returned slice);
 *    opaque handles have an explicit *_destroy.
 *  - Every function returns a zigz_status; the codes map 1:1 onto the Zig error names.
 *  - No global state: all state lives in a zigz_ctx (one per thread / per GPU).  A context is
 *    bound to one HIP device and one stream; calls on one context must not race.
 *  - Device-resident variants (zigz_dev_*) take device pointers to packed u32 canonical elements
 *    (4 B/element in HBM) and run on the context's stream; plain pointers, no torch types.
 *  - The library never falls back to the CPU for field or hash work: without a usable gfx950
 *    device zigz_ctx_create fails with ZIGZ_ERR_NO_DEVICE.
 */
#ifndef ZIGZ_HIP_H
#define ZIGZ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZIGZ_BABYBEAR_P 2013265921ull
#define ZIGZ_NUM_COLUMNS 43 /* src/prover/prover.zig:376-390 */
#define ZIGZ_HASH_SIZE 32   /* src/commitments/merkle_tree.zig:24 */
#define ZIGZ_ABI_VERSION 1

typedef int32_t zigz_status;
enum {
    ZIGZ_OK = 0,
    ZIGZ_ERR_EMPTY_EVALUATIONS = 1,         /* error.EmptyEvaluations      multilinear.zig:37-39 */
    ZIGZ_ERR_LENGTH_NOT_POWER_OF_TWO = 2,   /* error.LengthNotPowerOfTwo   multilinear.zig:42-44 */
    ZIGZ_ERR_WRONG_NUMBER_OF_VARIABLES = 3, /* error.WrongNumberOfVariables multilinear.zig:111-113 */
    ZIGZ_ERR_NO_VARIABLES_TO_FIX = 4,       /* error.NoVariablesToFix      multilinear.zig:155-157 */
    ZIGZ_ERR_NO_VARIABLES = 5,              /* error.NoVariables           multilinear.zig:206-208 */
    ZIGZ_ERR_PROTOCOL_ERROR = 6,            /* error.ProtocolError         sumcheck_prover.zig:80-82 */
    ZIGZ_ERR_EMPTY_VALUES = 7,              /* error.EmptyValues           merkle_tree.zig:284 */
    ZIGZ_ERR_TOO_MANY_VALUES = 8,           /* error.TooManyValues         merkle_tree.zig:287 */
    ZIGZ_ERR_INDEX_OUT_OF_BOUNDS = 9,       /* error.IndexOutOfBounds      merkle_tree.zig:325 */
    ZIGZ_ERR_POINT_DIMENSION_MISMATCH = 10, /* error.PointDimensionMismatch polynomial_commit.zig:92-94 */
    ZIGZ_ERR_NO_QUERIES = 11,               /* error.NoQueries             lasso_prover.zig:108-110 */
    ZIGZ_ERR_TOO_MANY_QUERIES = 12,         /* error.TooManyQueries        lasso_prover.zig:131 */
    ZIGZ_ERR_MAPPING_LENGTH_MISMATCH = 13,  /* error.MappingLengthMismatch lasso_prover.zig:185-187 */
    ZIGZ_ERR_INVALID_MAPPING = 14,          /* error.InvalidMapping        lasso_prover.zig:191-193 */
    ZIGZ_ERR_QUERY_TABLE_MISMATCH = 15,     /* error.QueryTableMismatch    lasso_prover.zig:198-200 */
    ZIGZ_ERR_EMPTY_TRACE = 16,              /* error.EmptyTrace            prover.zig:147-149 */
    ZIGZ_ERR_OUT_OF_MEMORY = 17,            /* error.OutOfMemory (host or device) */
    ZIGZ_ERR_WRONG_NUMBER_OF_CHALLENGES = 18, /* error.WrongNumberOfChallenges sumcheck_prover.zig:105-107 */
    /* backend-specific (no Zig counterpart) */
    ZIGZ_ERR_NO_DEVICE = 100,     /* no HIP device / not gfx950 / kernels not loadable */
    ZIGZ_ERR_HIP = 101,           /* a HIP runtime call failed; see zigz_last_error */
    ZIGZ_ERR_NOT_CANONICAL = 102, /* a field element >= p crossed the boundary */
    ZIGZ_ERR_INVALID_ARGUMENT = 103,
    ZIGZ_ERR_BAD_STATE = 104,     /* commit-job calls out of order */
    ZIGZ_ERR_COMM = 105           /* a sharded proof's exchange hook failed, or another rank reported an error */
};

typedef struct zigz_ctx zigz_ctx;
typedef struct zigz_merkle zigz_merkle;         /* one committed column: all tree levels in HBM */
typedef struct zigz_commit_job zigz_commit_job; /* a batch of columns going through commit -> open */
typedef struct zigz_transcript zigz_transcript; /* host-side SHA3 Fiat-Shamir sponge */
typedef struct zigz_merkle_batch zigz_merkle_batch; /* k committed tables: their values and trees in one allocation */

/* ---------------------------------------------------------------- context */
uint32_t zigz_abi_version(void);
const char *zigz_status_name(zigz_status s); /* the Zig error name, e.g. "LengthNotPowerOfTwo" */
zigz_status zigz_device_count(int *count);
/* Binds a context to HIP device `device` (must be gfx950) and creates its stream + workspace. */
zigz_status zigz_ctx_create(int device, zigz_ctx **out);
/* How host threads of this process wait for the device (stream / event synchronisation inside the calls below): on != 0
 * they sleep until the device signals instead of spinning.  For a host that keeps more proofs in flight than it has cores
 * (one thread per proof, most of them waiting for the GPU or for the sponge service); costs a wake-up per wait, so leave it
 * off for a lone proof.  Call before the contexts of `device` are created.  With it on, the two waits of a commit job
 * (zigz_commit_roots, zigz_commit_open_all) do not use the runtime's wait at all: the last kernel stores a completion word
 * into pinned memory next to the results it wrote there, and the thread looks at it between sleeps of 30-150 us (the
 * runtime's interrupt wait costs 0.2-0.5 ms of CPU per wait once tens of threads wait at once). */
zigz_status zigz_device_set_blocking_sync(int device, int on);
void zigz_ctx_destroy(zigz_ctx *ctx);
const char *zigz_last_error(const zigz_ctx *ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream); NULL restores the own stream. */
zigz_status zigz_ctx_set_stream(zigz_ctx *ctx, void *hip_stream);
void *zigz_ctx_get_stream(zigz_ctx *ctx);
zigz_status zigz_ctx_synchronize(zigz_ctx *ctx);
/* Device memory for callers without their own allocator (hipMalloc / hipFree). */
zigz_status zigz_dev_alloc(zigz_ctx *ctx, size_t bytes, void **d_out);
zigz_status zigz_dev_free(zigz_ctx *ctx, void *d_ptr);
/* Gives the context's workspaces back to the device (they are grown on demand and otherwise kept for the life of the
 * context: trees, lists, staging).  For a host that has just put an unusually large job through a context it keeps many of;
 * what the context learnt about its traces (the room its lists need) stays.  ZIGZ_ERR_BAD_STATE while a commit job is active. */
zigz_status zigz_ctx_release_workspaces(zigz_ctx *ctx);
/* free / total HBM of the context's device (hipMemGetInfo): a service sizes its number of proofs in flight from it */
zigz_status zigz_dev_mem_info(zigz_ctx *ctx, size_t *free_bytes, size_t *total_bytes);
/* canonical u64 host -> packed u32 device (validates < p), and back */
zigz_status zigz_dev_upload_u64(zigz_ctx *ctx, const uint64_t *h_in, size_t n, uint32_t *d_out);
zigz_status zigz_dev_download_u64(zigz_ctx *ctx, const uint32_t *d_in, size_t n, uint64_t *h_out);

/* ---------------------------------------------------------------- Multilinear(F), host buffers
 * Drop-in for src/poly/multilinear.zig; `in` is `self.evaluations` (len n = 2^v). */
/* partialEval(self, r, allocator) !Self   multilinear.zig:154-180: out[i]=(1-r)a[i]+r*a[i+n/2], i<n/2 */
zigz_status zigz_mle_bind(zigz_ctx *ctx, const uint64_t *in, size_t n, uint64_t r, uint64_t *out);
/* roundPolynomial(self, allocator) ![]F   multilinear.zig:205-232: out = [s0, s1 - s0] */
zigz_status zigz_mle_round_poly(zigz_ctx *ctx, const uint64_t *in, size_t n, uint64_t out[2]);
/* sumOverHypercube(self) F                multilinear.zig:188-194 */
zigz_status zigz_mle_sum(zigz_ctx *ctx, const uint64_t *in, size_t n, uint64_t *out);
/* eval(self, point) !F                    multilinear.zig:110-144 (point[0] <-> LSB of the index) */
zigz_status zigz_mle_eval(zigz_ctx *ctx, const uint64_t *in, size_t n, const uint64_t *point,
                          size_t point_len, uint64_t *out);

/* ---------------------------------------------------------------- SumcheckProver(F)
 * prove(poly, allocator) !Proof           src/proofs/sumcheck_prover.zig:26-91
 * rounds: 2*v values [c0,c1] per round; point: v challenges in binding order; SHA3 transcript
 * (fresh per call, src/proofs/sumcheck_protocol.zig:161,176-184) runs on the host inside. */
zigz_status zigz_sumcheck_prove(zigz_ctx *ctx, const uint64_t *in, size_t n, uint64_t *rounds,
                                uint64_t *point, uint64_t *final_eval);
/* proveInteractive(poly, challenges, allocator)  sumcheck_prover.zig:97-144 */
zigz_status zigz_sumcheck_prove_interactive(zigz_ctx *ctx, const uint64_t *in, size_t n,
                                            const uint64_t *challenges, size_t n_challenges,
                                            uint64_t *rounds, uint64_t *point, uint64_t *final_eval);

/* ---------------------------------------------------------------- SimpleMerkleTree(F, SHA3Hasher)
 * build(values, allocator) !Self          src/commitments/merkle_tree.zig:283-318 (pads with hashLeaf(0)) */
zigz_status zigz_merkle_commit(zigz_ctx *ctx, const uint64_t *values, size_t n, uint8_t root[32],
                               size_t *height, zigz_merkle **out);
/* open(self, index) !OpeningProof(F)      merkle_tree.zig:324-360; siblings: 32*height B, dirs: height B */
zigz_status zigz_merkle_open(zigz_ctx *ctx, const zigz_merkle *tree, size_t index, uint8_t *siblings,
                             uint8_t *dirs, uint64_t *leaf_value);
void zigz_merkle_destroy(zigz_ctx *ctx, zigz_merkle *tree);
/* CommitmentScheme.open(poly, tree, point, allocator) !Proof   src/commitments/polynomial_commit.zig:86-115
 * = eval(point) + tree.open(point[0].value mod 2^v)  (pointToIndex, :178-183) */
zigz_status zigz_commit_open(zigz_ctx *ctx, const uint64_t *evals, size_t n, const zigz_merkle *tree,
                             const uint64_t *point, size_t point_len, uint64_t *value, uint64_t *index,
                             uint8_t *siblings, uint8_t *dirs, uint64_t *leaf_value);

/* ---------------------------------------------------------------- Prover.generateCommitments (batched)
 * src/prover/prover.zig:366-467, split at the two transcript dependencies so the caller keeps its
 * own Fiat-Shamir transcript:  begin (Merkle builds, async) -> roots -> [caller absorbs roots, draws
 * ncols*v challenges] -> open_all (evals + paths) -> end.
 * cols: column-major, column c at cols + c*col_stride (elements), each 2^nv long. */
zigz_status zigz_commit_begin(zigz_ctx *ctx, const uint64_t *cols, size_t ncols, size_t col_stride,
                              size_t nv, zigz_commit_job **out);
/* device-resident columns (packed u32 canonical); the buffer must stay valid until zigz_commit_end */
zigz_status zigz_commit_begin_dev(zigz_ctx *ctx, const uint32_t *d_cols, size_t ncols, size_t col_stride,
                                  size_t nv, zigz_commit_job **out);
/* Several proofs in ONE job (a proving service with many SMALL traces: the reference's own tests and examples prove 4 .. 64
 * steps, tests/integration_tests.zig:171-206, BASELINE config 2 is 2^16 -- sizes at which a proof's ~35 launches are mostly
 * latency).  d_cols[z]: proof z's `ncols` device-resident columns (stride col_stride), all proofs 2^nv rows; nproofs <= 32,
 * nproofs * ncols <= 4096.  The job then behaves like one of nproofs * ncols columns numbered proof by proof: roots, points,
 * values, indices, leaves, siblings and dirs of proof z occupy the positions [z * ncols, (z + 1) * ncols) of the arrays of
 * zigz_commit_roots / zigz_commit_open_all; every proof's results are the ones its own job would give.  The columns are
 * copied at begin (the callers' buffers are not needed after it returns ... after the stream has passed the copy:
 * zigz_commit_roots).  2^nv < 2^15: the proofs' trees are built densely like any table's; 2^15 <= 2^nv <= 2^18: with the
 * structure-aware levels (option "batch_reserve" = n sizes the context's workspace for n proofs from its first batched job on, so
 * that a larger batch than any before does not reallocate gigabytes in the middle of a service's work), every column of a proof must then be hinted ("run_aware_mask" / "cons_group_mask" cover all of
 * them, as the witness's 43 are in host/prover.cpp), else ZIGZ_ERR_INVALID_ARGUMENT; larger tables: one job per proof. */
zigz_status zigz_commit_begin_batch(zigz_ctx *ctx, const uint32_t *const *d_cols, size_t nproofs, size_t ncols,
                                    size_t col_stride, size_t nv, zigz_commit_job **out);
/* zigz_commit_begin* ENQUEUES the Merkle builds and returns (nothing on that path is read back by the host: ~0.15 ms for the
 * ~45 launches of a 2^20 x 43 job); zigz_commit_roots waits for them; roots: ncols*32 bytes (prover.zig:405-410).
 * One job per context at a time (a second begin returns ZIGZ_ERR_BAD_STATE).  Other calls on the same context
 * between begin and end are allowed -- e.g. a Zig host evaluating one MLE while the trees build: they queue behind
 * the builds on the context's stream, and the job's roots travel through a pinned buffer of their own, so they
 * arrive intact (tests/test_gpu_parity.py::test_commit_job_survives_interleaved_calls). */
zigz_status zigz_commit_roots(zigz_commit_job *job, uint8_t *roots);
/* points: ncols*nv challenges (row c = point of column c).  Outputs per column: value = eval(point)
 * (prover.zig:427), index = point[0] mod 2^nv, leaf = evaluations[index], siblings ncols*nv*32 B,
 * dirs ncols*nv B (prover.zig:431 -> polynomial_commit.zig:86-115 -> merkle_tree.zig:324-360). */
zigz_status zigz_commit_open_all(zigz_commit_job *job, const uint64_t *points, uint64_t *values,
                                 uint64_t *indices, uint64_t *leaves, uint8_t *siblings, uint8_t *dirs);
/* k openings of the job's trees in shared launches: cols[j] in the job's column numbering (proof by proof for a batched job),
 * indices[j] < 2^nv.  All paths have nv levels: opening j at siblings + j*nv*32, dirs + j*nv; leaf_values[j] is the column's
 * cell at indices[j].  Valid once zigz_commit_roots has returned ZIGZ_OK for the job and until zigz_commit_end
 * (ZIGZ_ERR_BAD_STATE otherwise); before or after zigz_commit_open_all, whose results it does not change.  Host outputs.
 * k <= ZIGZ_VERIFY_BATCH_MAX; k == 0: ZIGZ_OK, nothing touched; cols[j] >= the job's columns: ZIGZ_ERR_INVALID_ARGUMENT,
 * indices[j] >= 2^nv: ZIGZ_ERR_INDEX_OUT_OF_BOUNDS, the first such j to *bad_index (if non-NULL), nothing written. */
zigz_status zigz_commit_open_many(zigz_commit_job *job, size_t k, const uint32_t *cols, const uint64_t *indices,
                                  uint8_t *siblings, uint8_t *dirs, uint64_t *leaf_values, size_t *bad_index);
/* diagnostic (tests): device address of the job's trees once built -- per column `bytes_per_column` = 2 * 2^nv nodes x 32 B
 * in the kernels' internal node form (level l at node offset 2N - 2(N >> l)); valid until zigz_commit_end.  Lets a test
 * compare two builds of the same columns node for node (dense vs table / run-aware / content-addressed levels).  Whole
 * node-addressed trees exist only when no column is list-built or the job was begun with "run_aware_materialize" = 1:
 * ZIGZ_ERR_BAD_STATE otherwise. */
zigz_status zigz_commit_job_tree(zigz_commit_job *job, const void **d_tree, size_t *bytes_per_column);
void zigz_commit_end(zigz_commit_job *job);

/* ---------------------------------------------------------------- LassoProver(F)
 * prove(table, queries, allocator) !Proof   src/lookups/lasso_prover.zig:103-173
 * table / queries: row-major, each row = n_in input fields then n_out output fields.
 * Outputs: nv = log2(ceilPow2(n_queries)); rounds 2*nv; point nv; the two flat SHA3 commitments. */
zigz_status zigz_lasso_prove(zigz_ctx *ctx, const uint64_t *table, size_t table_rows, const uint64_t *queries,
                             size_t n_queries, size_t n_in, size_t n_out, size_t *nv_out, uint64_t *rounds,
                             uint64_t *point, uint64_t *final_eval, uint8_t query_commitment[32],
                             uint8_t table_commitment[32]);
/* proveWithMapping(table, queries, mapping, allocator)   lasso_prover.zig:179-205 */
zigz_status zigz_lasso_prove_with_mapping(zigz_ctx *ctx, const uint64_t *table, size_t table_rows,
                                          const uint64_t *queries, size_t n_queries, size_t n_in, size_t n_out,
                                          const uint64_t *mapping, size_t n_mapping, size_t *nv_out,
                                          uint64_t *rounds, uint64_t *point, uint64_t *final_eval,
                                          uint8_t query_commitment[32], uint8_t table_commitment[32]);
/* hashEntry / hashQuery fingerprints (lasso_prover.zig:208-239) for `rows` rows of `width` fields */
zigz_status zigz_lasso_fingerprints(zigz_ctx *ctx, const uint64_t *rows_in, size_t rows, size_t width,
                                    uint64_t *out);

/* ---------------------------------------------------------------- witness columns (K8)
 * F.init(u64) = x mod p over raw 64-bit trace words (src/constraints/witness.zig:76,112,164-170,237-239):
 * d_out[i] = h_in[i] mod p, packed u32, for building device-resident columns from raw trace data. */
zigz_status zigz_dev_reduce_u64(zigz_ctx *ctx, const uint64_t *h_in, size_t n, uint32_t *d_out);
/* WitnessGenerator.generate on the device   src/constraints/witness.zig:29-270, column order prover.zig:376-390.
 * h_rows: the execution trace as packed rows, [num_steps][43] raw 64-bit words in column order (pc, x0..x31,
 * opcode, rd, rs1, rs2, funct3, funct7, imm as u64(bitcast i64), mem address, mem value, is_read).  Builds the 43
 * padded columns of 2^nv packed-u32 cells (nv = log2_int_ceil(num_steps)) at d_cols + c*col_stride. */
zigz_status zigz_dev_witness_from_rows(zigz_ctx *ctx, const uint64_t *h_rows, size_t num_steps, size_t nv,
                                       uint32_t *d_cols, size_t col_stride);

/* The same columns from the COMPACT trace: one 48-byte record per executed step instead of its 43 raw words (344 B).
 * A `Step` of src/vm/trace.zig:73-97 carries two full register files, but regs_after differs from the previous step's
 * in at most the one register the instruction wrote (src/vm/state.zig:188-597: every instruction writes <= 1 register;
 * x0 never changes, src/vm/registers.zig:38-48), so a step is: pc, the instruction's decoded fields, the register
 * write (wr_reg, rd_value) and the memory access.  The device rebuilds the 32 register columns by carrying each
 * register's last written value forward (witness.zig:65-123), reduces every cell mod p (F.init, witness.zig:76,112,
 * 164-170,237-239) and applies the padding rule (pc and registers repeat their last value, the rest is 0:
 * witness.zig:80-87,116-123).  A Zig host fills one record per trace.steps.items[i]:
 *   pc = step.pc; opcode..funct7, imm = step.instruction.*; (wr_reg, rd_value) = the r with regs_after[r] != regs_before[r]
 *   (0 when none); mem_* = step.memory_access (zeros / mem_is_read = 0 when null; mem_is_read = 1 for .Load). */
typedef struct zigz_trace_step {
    uint64_t pc;        /* step.pc */
    uint64_t rd_value;  /* regs_after[wr_reg]; ignored when wr_reg == 0 */
    uint64_t mem_addr;  /* memory_access.address (0 when none) */
    uint64_t mem_value; /* memory_access.value   (0 when none) */
    int64_t imm;        /* instruction.imm */
    uint8_t opcode, rd, rs1, rs2, funct3, funct7; /* @intFromEnum(opcode) and the raw fields, witness.zig:164-169 */
    uint8_t wr_reg;      /* 1..31: the register this step wrote; 0 (or any value >= 32): none */
    uint8_t mem_is_read; /* 1 = load, 0 = store or no access */
} zigz_trace_step;
/* initial_regs: the 32 register values before the first step (NULL = all zero); x0 is forced to 0.  h_steps may be
 * pageable or pinned (zigz_host_register) memory; the call returns when the copy has completed. */
zigz_status zigz_dev_witness_from_steps(zigz_ctx *ctx, const zigz_trace_step *h_steps, size_t num_steps, size_t nv,
                                        const uint64_t *initial_regs, uint32_t *d_cols, size_t col_stride);
/* The same, without waiting: copy, expansion and whatever the caller enqueues next (zigz_commit_begin_dev on d_cols)
 * run on the context's stream underneath the host's transcript work.  h_steps MUST be page-locked (zigz_host_register)
 * and stay unmodified until the stream has passed the copy (zigz_commit_roots / zigz_ctx_synchronize). */
zigz_status zigz_dev_witness_from_steps_async(zigz_ctx *ctx, const zigz_trace_step *h_steps, size_t num_steps, size_t nv,
                                              const uint64_t *initial_regs, uint32_t *d_cols, size_t col_stride);
/* The asynchronous form into a column buffer the CONTEXT owns (a workspace, reused call after call: nothing is allocated
 * on the steady-state path of a service that proves trace after trace on a pool of contexts).  *d_cols / *col_stride are
 * valid until the next call of this function, zigz_commit_begin (host columns), zigz_bench_kernel or
 * zigz_ctx_release_workspaces on the context -- in particular through a commit job begun on them. */
zigz_status zigz_dev_witness_from_steps_ws(zigz_ctx *ctx, const zigz_trace_step *h_steps, size_t num_steps, size_t nv,
                                           const uint64_t *initial_regs, const uint32_t **d_cols, size_t *col_stride);
/* The 32-BYTE record (what crosses PCIe per step decides the rate of a service whose traces arrive from the host: 48 B per step
 * are 50 MB per 2^20 proof).  Two observations about src/vm/trace.zig:73-97: instruction.imm is a sign-extended field of at
 * most 32 bits in every RV64IM format (src/isa/rv64i.zig:156-233), and memory_access is null on every step that is not a
 * LOAD / STORE.  So: imm as i32, and the memory triple in a SIDE LIST of zigz_mem_access (16 B per access) that a step refers
 * to by index -- ZIGZ_NO_MEM_ACCESS on the steps without one (an index >= num_mem reads as "none" as well).  mem_is_read
 * stays in the record.  A kernel widens the records on the device (zigz_trace_step, above) and the same expansion follows:
 * identical columns (tests/test_gpu_parity.py: both records against the numpy restatement and the oracle). */
typedef struct zigz_trace_step32 {
    uint64_t pc;        /* step.pc */
    uint64_t rd_value;  /* regs_after[wr_reg]; ignored when wr_reg == 0 */
    int32_t imm;        /* instruction.imm (sign-extended to i64 on the device) */
    uint32_t mem_index; /* index of this step's access in the side list, or ZIGZ_NO_MEM_ACCESS */
    uint8_t opcode, rd, rs1, rs2, funct3, funct7;
    uint8_t wr_reg;      /* 1..31: the register this step wrote; 0 (or any value >= 32): none */
    uint8_t mem_is_read; /* 1 = load, 0 = store or no access */
} zigz_trace_step32;
typedef struct zigz_mem_access {
    uint64_t addr, value; /* memory_access.address / .value */
} zigz_mem_access;
#define ZIGZ_NO_MEM_ACCESS 4294967295
/* as zigz_dev_witness_from_steps (waits for the copies) */
zigz_status zigz_dev_witness_from_steps32(zigz_ctx *ctx, const zigz_trace_step32 *h_steps, size_t num_steps,
                                          const zigz_mem_access *h_mem, size_t num_mem, size_t nv, const uint64_t *initial_regs,
                                          uint32_t *d_cols, size_t col_stride);
/* as zigz_dev_witness_from_steps_ws (asynchronous, into the context's own column buffer; page-locked records) */
zigz_status zigz_dev_witness_from_steps32_ws(zigz_ctx *ctx, const zigz_trace_step32 *h_steps, size_t num_steps,
                                             const zigz_mem_access *h_mem, size_t num_mem, size_t nv, const uint64_t *initial_regs,
                                             const uint32_t **d_cols, size_t *col_stride);
/* The 16-BYTE record.  One more observation about src/vm/trace.zig:73-97: the seven instruction fields of a step (opcode, rd, rs1,
 * rs2, funct3, funct7, imm) are the decoded instruction AT step.pc (src/vm/state.zig:128-140: fetch, decode, execute) -- a
 * program of P instructions has P different field tuples however long it runs.  So the fields travel ONCE per instruction, in a
 * code table indexed by (pc - code_base) / 4, and a step carries where it was, what it wrote and which access it made:
 *   pc_word : (pc - code_base) with mem_is_read in bit 0 (pc - code_base is a multiple of 4 below 2^32: RV64IM has no 16-bit forms)
 *   mem_wr  : bits 0-26 the index of the step's access in the side list (ZIGZ_NO_MEM_ACCESS16 = none; an index >= num_mem reads as
 *             none as well), bits 27-31 wr_reg
 * A caller whose trace does not fit -- a pc that is not 4-aligned or 2^32 past the base, the same pc executed with two different
 * decodings (a program that rewrote itself), 2^27 - 1 or more accesses -- uses the 32-byte record (the host mirror does: host/capi.cpp).
 * A step whose pc_word points past the table gets zero fields.  The kernel widens to zigz_trace_step and the same expansion
 * follows: identical columns (tests/test_gpu_parity.py).  16.8 MB instead of 33.6 cross PCIe for a 2^20 trace of a loop. */
typedef struct zigz_trace_step16 {
    uint32_t pc_word;
    uint32_t mem_wr;
    uint64_t rd_value;  /* regs_after[wr_reg]; ignored when wr_reg == 0 */
} zigz_trace_step16;
typedef struct zigz_code_entry {
    int32_t imm;        /* instruction.imm (sign-extended to i64 on the device) */
    uint8_t opcode, rd, rs1, rs2, funct3, funct7;
    uint8_t reserved0, reserved1; /* 0 */
} zigz_code_entry;
#define ZIGZ_NO_MEM_ACCESS16 134217727
/* as zigz_dev_witness_from_steps32 (waits for the copies) */
zigz_status zigz_dev_witness_from_steps16(zigz_ctx *ctx, const zigz_trace_step16 *h_steps, size_t num_steps,
                                          const zigz_mem_access *h_mem, size_t num_mem, uint64_t code_base,
                                          const zigz_code_entry *h_code, size_t num_code, size_t nv, const uint64_t *initial_regs,
                                          uint32_t *d_cols, size_t col_stride);
/* as zigz_dev_witness_from_steps32_ws (asynchronous, into the context's own column buffer; page-locked records, side list and table) */
zigz_status zigz_dev_witness_from_steps16_ws(zigz_ctx *ctx, const zigz_trace_step16 *h_steps, size_t num_steps,
                                             const zigz_mem_access *h_mem, size_t num_mem, uint64_t code_base,
                                             const zigz_code_entry *h_code, size_t num_code, size_t nv, const uint64_t *initial_regs,
                                             const uint32_t **d_cols, size_t *col_stride);
/* Page-lock a host buffer the caller reuses for uploads (trace records, witness columns): H2D copies from registered
 * memory run at PCIe rate without the staging copy.  zigz_host_unregister before freeing the buffer; page-locking belongs
 * to the process, so unregister accepts ctx == NULL (the registering context may already be destroyed). */
zigz_status zigz_host_register(zigz_ctx *ctx, void *h_ptr, size_t bytes);
zigz_status zigz_host_unregister(zigz_ctx *ctx, void *h_ptr);

/* ---------------------------------------------------------------- device-resident MLE / sumcheck */
zigz_status zigz_dev_mle_bind(zigz_ctx *ctx, const uint32_t *d_in, size_t n, uint64_t r, uint32_t *d_out);
/* fused: d_out = bind(d_in, r) and sums[0..1] = (sum of low half, sum of high half) of d_out */
zigz_status zigz_dev_mle_bind_sums(zigz_ctx *ctx, const uint32_t *d_in, size_t n, uint64_t r, uint32_t *d_out,
                                   uint64_t half_sums[2]);
zigz_status zigz_dev_mle_half_sums(zigz_ctx *ctx, const uint32_t *d_in, size_t n, uint64_t half_sums[2]);
zigz_status zigz_dev_mle_eval(zigz_ctx *ctx, const uint32_t *d_in, size_t n, const uint64_t *point,
                              size_t point_len, uint64_t *out);
/* d_scratch: n/2 + n/4 ... < n elements of scratch (may be NULL: taken from the context workspace) */
zigz_status zigz_dev_sumcheck_prove(zigz_ctx *ctx, const uint32_t *d_in, size_t n, uint32_t *d_scratch,
                                    const uint64_t *fixed_challenges, uint64_t *rounds, uint64_t *point,
                                    uint64_t *final_eval);

/* ---------------------------------------------------------------- one sumcheck over several GPUs (row sharding)
 * SumcheckProver.prove (src/proofs/sumcheck_prover.zig:26-91) of ONE table of n = n_local * world elements, element i on
 * rank i mod world at local index i / world (so every MSB-first bind pair of partialEval, multilinear.zig:166-173, is
 * rank-local).  Radix form: per stage of k <= 10 rounds the ranks exchange 2^k exact u64 partial block sums, then one
 * exchange re-assembles the last <= 1024 * world entries: 2-3 exchanges per proof, all through `allgather` (every rank
 * contributes `bytes` from `send`; `recv` gets world * bytes in rank order; return 0 on success -- bind it to RCCL,
 * MPI or torch.distributed).  Every rank returns the same rounds / point / final_eval as the unsharded prover.
 * Failure is collective: every payload carries one status word, so a rank whose local pass failed (HIP error, a callback's
 * status) takes part in the next exchange with that status and ALL ranks stop there -- the failing rank returns its own
 * error, the others ZIGZ_ERR_COMM -- instead of waiting for the transport's timeout; a hook that returns nonzero is
 * ZIGZ_ERR_COMM as well. */
typedef int (*zigz_allgather_fn)(void *user, const void *send, size_t bytes, void *recv);
zigz_status zigz_dev_sumcheck_prove_sharded(zigz_ctx *ctx, const uint32_t *d_local, size_t n_local, int rank, int world,
                                            zigz_allgather_fn allgather, void *user, uint64_t *rounds, uint64_t *point,
                                            uint64_t *final_eval);
/* Built-in zigz_allgather_fn for the ranks of ONE node: a mailbox in POSIX shared memory.  What the sharded provers
 * exchange is host-resident (it was read back for the SHA3 transcript) and <= 64 KiB, so between processes of a node
 * this is the shortest path (a few microseconds per exchange); across nodes bind the hook to RCCL / MPI.  Every rank
 * calls create with the same job-unique `name` (<= 80 chars, no '/'), world and max_bytes (largest `bytes` of any
 * exchange); rank 0 creates the segment, the others attach (waiting up to timeout_s; <= 0: 60 s).  Creation is a
 * collective with a handshake: an attacher accepts a segment only once the live rank 0 has echoed the random token it
 * wrote there (a segment left behind by a crashed job under the same name has nobody to answer and is let go), and rank 0
 * returns when every rank has been acknowledged.  `name` must still be unique among jobs that START at the same time: put a
 * job id or a nonce broadcast by rank 0 into it.  Pass the comm as the hook's `user`.  A rank that waits longer than
 * timeout_s inside an exchange returns nonzero instead of hanging. */
typedef struct zigz_shm_comm zigz_shm_comm;
zigz_status zigz_shm_comm_create(const char *name, int rank, int world, size_t max_bytes, double timeout_s,
                                 zigz_shm_comm **out);
int zigz_shm_allgather(void *comm, const void *send, size_t bytes, void *recv);
void zigz_shm_comm_destroy(zigz_shm_comm *comm);
/* RCCL as the transport, without torch: for ranks on different GPUs of an xGMI node (or on several nodes).  The 128-byte
 * unique id comes from ONE rank (zigz_rccl_unique_id) and reaches the others however the host distributes small blobs
 * (a file, MPI, its own socket); every rank then creates its communicator for HIP device `device`.  max_bytes: the largest
 * `bytes` of any exchange.  librccl.so is loaded on first use; ZIGZ_ERR_NO_DEVICE when it cannot be.
 *  - zigz_rccl_allgather is a zigz_allgather_fn (user = the comm): host buffers, staged through pinned + device memory;
 *  - zigz_rccl_allreduce_u64 sums n u64 words over the ranks (host buffers); ..._dev does it in place on words already in
 *    HBM on the given hipStream_t, no staging and no synchronisation;
 *  - zigz_dev_sumcheck_prove_rccl is zigz_dev_sumcheck_prove_sharded with the partial block sums of every radix stage
 *    (k <= 10 rounds of round-polynomial sums, sumcheck_prover.zig:50-77) all-reduced in HBM on the context's stream --
 *    one RCCL all-reduce per stage of rounds -- and the last <= 1024 * world entries all-gathered through the comm.
 * RCCL itself never times out, so every wait behind a collective here has a deadline (zigz_rccl_comm_set_timeout, default
 * 120 s): when it passes -- a peer never entered the collective -- the communicator is aborted (ncclCommAbort), the call
 * returns nonzero / ZIGZ_ERR_COMM and every later call on that communicator fails at once.  Failure of a sharded proof is
 * collective here too: the all-reduce of a stage carries one extra word, the number of ranks whose local pass failed, so
 * all ranks leave the proof at the same collective (the failing one with its own error, the others with ZIGZ_ERR_COMM).
 * zigz_rccl_stream_wait is the deadline wait for a stream that holds a ..._dev collective; zigz_rccl_comm_abort aborts by
 * hand.  (ncclCommInitRank inside zigz_rccl_comm_create has no deadline: a rank that never calls create blocks the others.) */
#define ZIGZ_RCCL_UNIQUE_ID_BYTES 128
typedef struct zigz_rccl_comm zigz_rccl_comm;
zigz_status zigz_rccl_unique_id(uint8_t id[ZIGZ_RCCL_UNIQUE_ID_BYTES]);
zigz_status zigz_rccl_comm_create(int device, const uint8_t id[ZIGZ_RCCL_UNIQUE_ID_BYTES], int rank, int world,
                                  size_t max_bytes, zigz_rccl_comm **out);
int zigz_rccl_allgather(void *comm, const void *send, size_t bytes, void *recv);
int zigz_rccl_allreduce_u64(zigz_rccl_comm *comm, const uint64_t *send, size_t n, uint64_t *recv);
int zigz_rccl_allreduce_u64_dev(zigz_rccl_comm *comm, uint64_t *d_words, size_t n, void *hip_stream);
int zigz_rccl_stream_wait(zigz_rccl_comm *comm, void *hip_stream);
void zigz_rccl_comm_set_timeout(zigz_rccl_comm *comm, double seconds);
void zigz_rccl_comm_abort(zigz_rccl_comm *comm);
int zigz_rccl_comm_rank(const zigz_rccl_comm *comm);
int zigz_rccl_comm_world(const zigz_rccl_comm *comm);
void zigz_rccl_comm_destroy(zigz_rccl_comm *comm);
zigz_status zigz_dev_sumcheck_prove_rccl(zigz_ctx *ctx, const uint32_t *d_local, size_t n_local, zigz_rccl_comm *comm,
                                         uint64_t *rounds, uint64_t *point, uint64_t *final_eval);
/* The same orchestration over caller-supplied data passes on the local table (what the GPU passes of the call above do):
 * block_sums: exact u64 sums of the 2^k contiguous blocks of the current table; fold: current := sum_b w[b] *
 * current[b*m + i] (2^k canonical weights, m = length / 2^k) and, when k_next != 0, the 2^k_next block sums of the result;
 * read_tail: the current table (m canonical values).  Each returns a zigz_status.  No GPU is touched. */
typedef struct zigz_radix_ops {
    void *user;
    zigz_status (*block_sums)(void *user, unsigned k, uint64_t *sums);
    zigz_status (*fold)(void *user, unsigned k, const uint64_t *weights, unsigned k_next, uint64_t *next_sums);
    zigz_status (*read_tail)(void *user, size_t m, uint64_t *out);
} zigz_radix_ops;
zigz_status zigz_sumcheck_radix_run(const zigz_radix_ops *ops, size_t n_local, int rank, int world,
                                    zigz_allgather_fn allgather, void *comm_user, const uint64_t *fixed_challenges,
                                    uint64_t *rounds, uint64_t *point, uint64_t *final_eval);
/* ... over data passes whose sums are ALREADY the sums over all ranks (reduced inside the pass by a collective of its own,
 * as the passes of zigz_dev_sumcheck_prove_rccl do with RCCL): no exchange per stage.  A pass that fails -- or learns inside
 * its collective that a peer failed -- returns nonzero on every rank at the same stage; the run then skips the remaining
 * passes everywhere and all ranks leave through the tail exchange, which carries the status words. */
zigz_status zigz_sumcheck_radix_run_reduced(const zigz_radix_ops *ops, size_t n_local, int rank, int world,
                                            zigz_allgather_fn allgather, void *comm_user, const uint64_t *fixed_challenges,
                                            uint64_t *rounds, uint64_t *point, uint64_t *final_eval);

/* ---------------------------------------------------------------- batched provers: many independent tables per call
 * k independent SumcheckProver.prove calls (src/proofs/sumcheck_prover.zig:26-91) in shared launches: every radix pass
 * (block sums, fold) serves all tables still in play in ONE launch, and every table keeps its own fresh transcript
 * (src/proofs/sumcheck_protocol.zig:161).  Results are byte-identical to calling the single entry once per table, in
 * order.  Table i has ns[i] = 2^v_i elements.  Outputs are concatenated in table order: rounds (2*v_i per table), points
 * (v_i per table), final_evals[k].  fixed_challenges == NULL gives Fiat-Shamir; otherwise it holds sum(v_i) challenges
 * concatenated the same way (proveInteractive, sumcheck_prover.zig:97-144).
 * k <= ZIGZ_BATCH_MAX, else ZIGZ_ERR_INVALID_ARGUMENT; k == 0 returns ZIGZ_OK and touches nothing.  d_tables[i] must be
 * 16-byte aligned (ZIGZ_ERR_INVALID_ARGUMENT otherwise); the same table may appear more than once.  The arguments are
 * checked for every table before anything runs: on the first table (in index order) that the single entry would reject,
 * the call returns that same status, writes the table's index to *bad_index (if non-NULL) and launches nothing.
 * The batch always takes the radix schedule; the "per_round_sumcheck" option and timing mode do not apply to it. */
#define ZIGZ_BATCH_MAX 4096
zigz_status zigz_dev_sumcheck_prove_batch(zigz_ctx *ctx, const uint32_t *const *d_tables, const size_t *ns, size_t k,
                                          const uint64_t *fixed_challenges, uint64_t *rounds, uint64_t *points,
                                          uint64_t *final_evals, size_t *bad_index);
/* host buffers (canonical u64, checked as zigz_sumcheck_prove checks them), uploaded in one copy */
zigz_status zigz_sumcheck_prove_batch(zigz_ctx *ctx, const uint64_t *const *tables, const size_t *ns, size_t k,
                                      const uint64_t *fixed_challenges, uint64_t *rounds, uint64_t *points,
                                      uint64_t *final_evals, size_t *bad_index);
/* k LassoProver.prove / proveWithMapping calls (src/lookups/lasso_prover.zig:103-205): one upload of all rows, one
 * fingerprint launch over every table and query set, the query fingerprints proved in place by the batched sumcheck, and the
 * 2k flat commitments (:242-252) absorbed in lock step on the host underneath it.  Instance i is given by entry i of each
 * array, with the meaning of zigz_lasso_prove's arguments; mappings == NULL or mappings[i] == NULL: prove(), otherwise
 * proveWithMapping() with n_mappings[i] entries.  Outputs: nv_out[i], rounds[i] (2 * nv words, caller-allocated for
 * log2(ceilPow2(n_queries[i])) variables), points[i] (nv words), final_evals[i], and 32 bytes per instance at
 * query_commitments + 32 i / table_commitments + 32 i.  Errors: the status the single call would return for the first failing
 * instance, whose index goes to *bad_index (if non-NULL).  (Parallel arrays rather than a struct per instance: the binding
 * keeps the value structs it has.) */
zigz_status zigz_lasso_prove_batch(zigz_ctx *ctx, size_t k, const uint64_t *const *tables, const size_t *table_rows,
                                   const uint64_t *const *queries, const size_t *n_queries, const size_t *n_in,
                                   const size_t *n_out, const uint64_t *const *mappings, const size_t *n_mappings,
                                   size_t *nv_out, uint64_t *const *rounds, uint64_t *const *points, uint64_t *final_evals,
                                   uint8_t *query_commitments, uint8_t *table_commitments, size_t *bad_index);
/* The batched orchestration over caller-supplied data passes (the batched sibling of zigz_sumcheck_radix_run).  Each
 * callback serves `count` tables at once -- tables[j] is the index (into ns) of the j-th -- with inputs and outputs packed
 * in that order: block_sums writes the 2^k[j] exact u64 block sums of each current table; fold folds each current table
 * with its 2^k[j] canonical weights (current := sum_b w[b] * current[b*m + i], m = length / 2^k[j]) and, where k_next[j] != 0,
 * writes the 2^k_next[j] block sums of the result; read_tail writes each current table (m[j] canonical values).  Each
 * returns a zigz_status; the first that is not ZIGZ_OK ends the run with it.  No GPU is touched. */
typedef zigz_status (*zigz_radix_batch_sums_fn)(void *user, size_t count, const size_t *tables, const unsigned *k,
                                                uint64_t *sums);
typedef zigz_status (*zigz_radix_batch_fold_fn)(void *user, size_t count, const size_t *tables, const unsigned *k,
                                                const uint64_t *weights, const unsigned *k_next, uint64_t *next_sums);
typedef zigz_status (*zigz_radix_batch_tail_fn)(void *user, size_t count, const size_t *tables, const size_t *m, uint64_t *out);
zigz_status zigz_sumcheck_radix_run_batch(void *user, zigz_radix_batch_sums_fn block_sums, zigz_radix_batch_fold_fn fold,
                                          zigz_radix_batch_tail_fn read_tail, size_t k, const size_t *ns,
                                          const uint64_t *fixed_challenges, uint64_t *rounds, uint64_t *points,
                                          uint64_t *final_evals);

/* k independent SimpleMerkleTree.build calls (merkle_tree.zig:283-318; CommitmentScheme.batchCommit,
 * polynomial_commit.zig:132-157) in shared launches: ceil(max height / 9) build launches and one hand-off for the whole batch.
 * Table i has ns[i] >= 1 values of any length (padded with hashLeaf(0), like zigz_merkle_commit).  Outputs: roots (k * 32
 * bytes), heights[k]; every root is byte-identical to the single call's.  out == NULL: roots only (the trees are freed);
 * otherwise *out owns the values and trees of all k tables in ONE device allocation until zigz_merkle_batch_destroy.
 * The batch builds densely: the context's hint options, zigz_kernel_stats and an active commit job are neither read nor
 * changed (the calls queue behind the job on the context's stream).  k <= ZIGZ_BATCH_MAX, else ZIGZ_ERR_INVALID_ARGUMENT;
 * k == 0 returns ZIGZ_OK and touches nothing.  Every argument is checked before anything runs: on the first table the single
 * call would reject, the call returns that status, writes the table's index to *bad_index (if non-NULL), launches nothing
 * and leaves the outputs untouched.
 * Device form: d_values[i] are packed-u32 canonical values (not checked), 4-byte aligned; the same table may repeat. */
zigz_status zigz_dev_merkle_commit_batch(zigz_ctx *ctx, const uint32_t *const *d_values, const size_t *ns, size_t k,
                                         uint8_t *roots, size_t *heights, zigz_merkle_batch **out, size_t *bad_index);
/* host form: canonical u64 (ZIGZ_ERR_NOT_CANONICAL otherwise), uploaded in one copy */
zigz_status zigz_merkle_commit_batch(zigz_ctx *ctx, const uint64_t *const *values, const size_t *ns, size_t k,
                                     uint8_t *roots, size_t *heights, zigz_merkle_batch **out, size_t *bad_index);
/* tree_i.open(indices[i]) for every tree of the batch (merkle_tree.zig:324-360): siblings (32 B each) and dirs are packed
 * tree by tree, tree i at offset sum_{j<i} heights[j]; leaf_values[k].  One launch, one hand-off. */
zigz_status zigz_merkle_open_batch(zigz_ctx *ctx, const zigz_merkle_batch *b, const uint64_t *indices, uint8_t *siblings,
                                   uint8_t *dirs, uint64_t *leaf_values, size_t *bad_index);
/* tree_{trees[j]}.open(indices[j]) for j < k (merkle_tree.zig:324-360): any number of openings per tree, in any order, (tree,
 * index) pairs may repeat -- one launch per chunk of at most 32 MiB of results instead of one call per opening.  Outputs are
 * packed opening by opening in the layout zigz_merkle_verify_batch reads: opening j's siblings (32 B each) and dirs at offset
 * sum_{i<j} height(trees[i]); leaf_values[k]; roots (k * 32 B, may be NULL): the root of trees[j], so that the four arrays plus
 * heights are a complete argument list of the verify entries; heights (k, may be NULL).  Every opening is byte-identical to
 * zigz_merkle_open_batch's for that tree and index.  All checks run before anything is launched or written: k == 0 returns
 * ZIGZ_OK and touches nothing; ZIGZ_ERR_INVALID_ARGUMENT for ctx or b NULL, a b of another context, k > ZIGZ_VERIFY_BATCH_MAX,
 * trees or indices NULL, leaf_values NULL, siblings or dirs NULL unless every opening has height 0, trees[j] >= the batch's
 * table count; ZIGZ_ERR_INDEX_OUT_OF_BOUNDS for indices[j] >= the number of values of that table (zigz_merkle_open_batch's
 * rule); for the last two the first offending j goes to *bad_index (if non-NULL).  Leaves the hint options, zigz_kernel_stats,
 * an active commit job and other open batches alone. */
zigz_status zigz_merkle_open_many(zigz_ctx *ctx, const zigz_merkle_batch *b, size_t k, const uint32_t *trees,
                                  const uint64_t *indices, uint8_t *siblings, uint8_t *dirs, uint64_t *leaf_values,
                                  uint8_t *roots, size_t *heights, size_t *bad_index);
/* the same with siblings / dirs / leaf_values / roots written to DEVICE memory (d_siblings and d_roots 16-byte aligned,
 * d_leaf_values 8-byte aligned, else ZIGZ_ERR_INVALID_ARGUMENT); trees, indices and heights stay on the host.  Queues one
 * launch on the context's stream and returns; what it wrote is what zigz_dev_merkle_verify_batch takes. */
zigz_status zigz_dev_merkle_open_many(zigz_ctx *ctx, const zigz_merkle_batch *b, size_t k, const uint32_t *trees,
                                      const uint64_t *indices, uint8_t *d_siblings, uint8_t *d_dirs,
                                      uint64_t *d_leaf_values, uint8_t *d_roots, size_t *heights, size_t *bad_index);
/* CommitmentScheme.open(poly_i, tree_i, point_i) for every tree (polynomial_commit.zig:86-115): table i must have 2^v values
 * (ZIGZ_ERR_LENGTH_NOT_POWER_OF_TWO otherwise); points are concatenated, heights[i] canonical coordinates each; values[i] =
 * eval(point_i) over the stored values, indices[i] = pointToIndex(point_i) (:178-183), then the path as above.  One eval
 * launch, one path launch, one hand-off. */
zigz_status zigz_commit_open_batch(zigz_ctx *ctx, const zigz_merkle_batch *b, const uint64_t *points, uint64_t *values,
                                   uint64_t *indices, uint8_t *siblings, uint8_t *dirs, uint64_t *leaf_values,
                                   size_t *bad_index);
/* waits for the context's stream, then frees the batch (NULL: no-op) */
void zigz_merkle_batch_destroy(zigz_ctx *ctx, zigz_merkle_batch *b);
/* SimpleMerkleTree.verify (merkle_tree.zig:362-373) for k independent openings in shared launches; CommitmentScheme.batchVerify
 * (polynomial_commit.zig:160-175) is "*n_rejected == 0".  Opening i: roots[32 i..], heights[i] levels, leaf_values[i] (hashed as
 * its 8 little-endian bytes, like hashLeaf: values >= p are hashed as given), siblings (32 B each) and dirs packed opening by
 * opening at offset sum_{j<i} heights[j] (the layout zigz_merkle_open_batch / zigz_commit_open_batch write).  dirs[l] != 0:
 * the sibling is on the left (is_right).  Height 0: the check is hashLeaf(value) == root.  verdicts (k bytes, may be NULL):
 * 1 accept, 0 reject, bit for bit SimpleMerkleTree.verify; *n_rejected: the number of zeros.  What an opening holds never makes
 * an error: statuses are for the shape of the arguments only -- ZIGZ_ERR_INVALID_ARGUMENT for ctx or n_rejected NULL, a NULL
 * array when k > 0, k > ZIGZ_VERIFY_BATCH_MAX, or heights[i] > 64 (the first such i goes to *bad_index, if non-NULL), all
 * checked before anything runs.  k == 0: ZIGZ_OK, *n_rejected = 0, nothing else touched.  The call queues on the context's
 * stream and leaves the hint options, zigz_kernel_stats, an active commit job and open zigz_merkle_batch handles alone.
 * Host form: staged in chunks of at most 32 MiB through pinned memory (each bucket of one height level-major). */
#define ZIGZ_VERIFY_BATCH_MAX 4194304 /* 2^22 */
zigz_status zigz_merkle_verify_batch(zigz_ctx *ctx, size_t k, const uint8_t *roots, const size_t *heights,
                                     const uint64_t *leaf_values, const uint8_t *siblings, const uint8_t *dirs,
                                     uint8_t *verdicts, size_t *n_rejected, size_t *bad_index);
/* the same over device-resident roots / leaf_values / siblings / dirs (same layouts; d_roots and d_siblings 16-byte aligned,
 * d_leaf_values 8-byte aligned, else ZIGZ_ERR_INVALID_ARGUMENT); heights and the outputs stay on the host.  Option
 * "verify_pause" (A/B): 0 = hash with the re-arm pauses in launches of >= 4096 waves (default), 1 = always, 2 = never. */
zigz_status zigz_dev_merkle_verify_batch(zigz_ctx *ctx, size_t k, const uint8_t *d_roots, const size_t *heights,
                                         const uint64_t *d_leaf_values, const uint8_t *d_siblings, const uint8_t *d_dirs,
                                         uint8_t *verdicts, size_t *n_rejected, size_t *bad_index);

/* k independent Multilinear.eval calls (multilinear.zig:110-144; point[0] <-> LSB of the index) in shared launches: one launch
 * evaluates every (table, point) pair, a second hands the k results over.  Pair i: table i of ns[i] = 2^v_i elements and the v_i
 * coordinates at points + sum_{j<i} v_j (concatenated in pair order, like zigz_dev_sumcheck_prove_batch's points); out[i] is
 * byte-identical to zigz_dev_mle_eval(d_tables[i], ns[i], point_i, v_i) -- for ns[i] = 1 the table's one value.  The same
 * table may appear any number of times, with the same or different points.  k <= ZIGZ_BATCH_MAX, else
 * ZIGZ_ERR_INVALID_ARGUMENT; k == 0 returns ZIGZ_OK and touches nothing.  d_tables[i] must be 16-byte aligned, ns[i] <= 2^32 and
 * the call's tables together fewer than 2^24 chunks of 8192 elements, one launch's grid (ZIGZ_ERR_INVALID_ARGUMENT otherwise).  Every argument is checked for every pair before anything is launched or written: on
 * the first pair (in index order) that the single entry would reject, or whose point holds a coordinate >= p
 * (ZIGZ_ERR_NOT_CANONICAL), the call returns that status and writes the pair's index to *bad_index (if non-NULL).  Leaves the
 * hint options, zigz_kernel_stats, an active commit job and open zigz_merkle_batch handles alone; queues on the context's stream. */
zigz_status zigz_dev_mle_eval_batch(zigz_ctx *ctx, const uint32_t *const *d_tables, const size_t *ns, size_t k,
                                    const uint64_t *points, uint64_t *out, size_t *bad_index);
/* host tables (canonical u64, ZIGZ_ERR_NOT_CANONICAL with the pair's index otherwise), narrowed and uploaded in one copy;
 * zigz_mle_eval is the single entry */
zigz_status zigz_mle_eval_batch(zigz_ctx *ctx, const uint64_t *const *tables, const size_t *ns, size_t k,
                                const uint64_t *points, uint64_t *out, size_t *bad_index);
/* k independent SumcheckVerifier.verify calls (src/proofs/sumcheck_verifier.zig:48-108) whose oracle is the multilinear
 * extension of table i: the k oracle evaluations run in the batched eval's launch while the host replays the k transcripts.
 * Proof i, in the layout zigz_dev_sumcheck_prove_batch writes: ns[i] = 2^v_i, rounds (2 v_i words [c0, c1] per round) and
 * points (v_i words) concatenated in proof order, claimed_sums[i], final_evals[i].  Per proof, bit for bit the reference: a
 * fresh transcript, claim = claimed_sums[i]; per round reject if g(0) + g(1) != claim, absorb c0 and c1, draw the challenge
 * (sumcheck_protocol.zig:176-184), claim = g(challenge); then oracle_eval = eval(table_i, point_i) and the proof is accepted iff
 * oracle_eval == claim && oracle_eval == final_evals[i].
 * Outputs: verdicts[i] (may be NULL) 1 accept / 0 reject; *n_rejected the number of rejects; expected_evals[i] (may be NULL)
 * VerificationResult.expected_eval -- the claim at the failing round, or the final claim; oracle_evals[i] (may be NULL) the
 * evaluation, written for every proof including those whose rounds failed.
 * POINT ORDER.  flags == 0 evaluates the oracle at the proof's final point as given, point[0] <-> LSB, exactly as the reference's
 * verifier does.  The prover binds MSB-first, so with the proved table as the oracle an honest proof of two or more variables is
 * REJECTED in general -- that is the reference's behaviour and the default reproduces it.  ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED
 * evaluates at the reversed point, where the prover's final_eval lives: honest proofs are accepted.  (One variable: both agree.)
 * Statuses are for the shape of the arguments only, never for what a proof holds: ZIGZ_ERR_INVALID_ARGUMENT for ctx or
 * n_rejected NULL, an unknown flag, a NULL input array when k > 0, k > ZIGZ_BATCH_MAX, a table that is NULL, not 16-byte aligned
 * or larger than 2^32; the prover's rules per table (zigz_dev_sumcheck_prove: ns[i] = 1 is ZIGZ_ERR_NO_VARIABLES);
 * ZIGZ_ERR_NOT_CANONICAL for a point coordinate, round coefficient, claimed sum or final eval >= p.  All checked for every proof
 * before anything is launched or written; the first failing proof's index goes to *bad_index (if non-NULL).  k == 0: ZIGZ_OK,
 * *n_rejected = 0, nothing else touched.  Leaves alone what zigz_dev_mle_eval_batch leaves alone. */
#define ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED 1u
zigz_status zigz_dev_sumcheck_verify_batch(zigz_ctx *ctx, const uint32_t *const *d_tables, const size_t *ns, size_t k,
                                           const uint64_t *claimed_sums, const uint64_t *rounds, const uint64_t *points,
                                           const uint64_t *final_evals, uint32_t flags, uint8_t *verdicts,
                                           uint64_t *expected_evals, uint64_t *oracle_evals, size_t *n_rejected,
                                           size_t *bad_index);
/* host tables (canonical u64, ZIGZ_ERR_NOT_CANONICAL with the proof's index otherwise), narrowed and uploaded in one copy */
zigz_status zigz_sumcheck_verify_batch(zigz_ctx *ctx, const uint64_t *const *tables, const size_t *ns, size_t k,
                                       const uint64_t *claimed_sums, const uint64_t *rounds, const uint64_t *points,
                                       const uint64_t *final_evals, uint32_t flags, uint8_t *verdicts,
                                       uint64_t *expected_evals, uint64_t *oracle_evals, size_t *n_rejected,
                                       size_t *bad_index);

/* k independent sumchecks of a PRODUCT of multilinear tables in shared launches: instance i proves
 *   sum_{x in {0,1}^v_i} prod_{j < d_i} f_{i,j}(x),   d_i = degrees[i] in 1..ZIGZ_PRODUCT_MAX_DEGREE,
 * every factor of ns[i] = 2^v_i elements; d_factors holds sum d_i pointers, instance by instance.  This is SumcheckProver.prove
 * (src/proofs/sumcheck_prover.zig:26-91) with the round polynomial generalised: with a_j = f_j[x], b_j = f_j[x + m/2] (x < m/2)
 * the round's g(t) = sum_x prod_j (a_j + t (b_j - a_j)) in coefficient form c_0..c_d (the degree-2 and degree-3 round polynomials
 * the reference's proof format reserves, src/prover/proof.zig:61-77; the verifier is sumcheck_verifier.zig:172-205 with d + 1
 * coefficients).  The bind is partialEval's, MSB-first (multilinear.zig:166-173); every instance has a fresh transcript and per
 * round absorbs c_0..c_d in order, then draws the challenge (sumcheck_protocol.zig:176-184).  fixed_challenges != NULL is the
 * proveInteractive form: sum v_i challenges, concatenated in instance order, and no transcript.
 * Outputs, concatenated in instance order: claimed_sums[k] (the sum itself), rounds ((d_i + 1) v_i canonical words per
 * instance), points (v_i), factor_evals (d_i: each factor fully bound, i.e. its extension at the reversed point) and
 * final_evals[k] (their product).  For d_i = 1 rounds, points and final_evals are byte for byte what
 * zigz_dev_sumcheck_prove_batch writes for the same table.  There is no single-instance entry: k = 1 is the single.
 * Schedule: one data pass per round over every instance still longer than 1024 (at most one small copy and two launches per
 * round, whatever k is); the shorter tables finish on the host after one hand-off.  The caller's tables are only read: the same
 * table may serve as several factors of one instance (f * f) and in several instances.
 * Every argument is checked for every instance before anything is launched or written; the first failing instance's index goes
 * to *bad_index (if non-NULL): ZIGZ_ERR_INVALID_ARGUMENT for ctx or an array NULL, k > ZIGZ_BATCH_MAX, a degree outside
 * 1..ZIGZ_PRODUCT_MAX_DEGREE, a factor that is NULL or not 16-byte aligned, ns[i] > 2^ZIGZ_PRODUCT_MAX_LOG2_N (the exact u64
 * sums); ZIGZ_ERR_NO_VARIABLES for ns[i] == 1; ZIGZ_ERR_LENGTH_NOT_POWER_OF_TWO; ZIGZ_ERR_NOT_CANONICAL for a fixed challenge
 * >= p.  The instances longer than 1024 must together make fewer than 2^24 chunks of 8192 elements, one launch's grid
 * (ZIGZ_ERR_INVALID_ARGUMENT otherwise, before anything is launched).  k == 0 returns ZIGZ_OK and touches nothing.  Leaves the hint options, zigz_kernel_stats, an active commit job and open
 * zigz_merkle_batch handles alone; queues on the context's stream. */
#define ZIGZ_PRODUCT_MAX_DEGREE 3
#define ZIGZ_PRODUCT_MAX_LOG2_N 30
zigz_status zigz_dev_sumcheck_prove_product_batch(zigz_ctx *ctx, size_t k, const unsigned *degrees,
                                                  const uint32_t *const *d_factors, const size_t *ns,
                                                  const uint64_t *fixed_challenges, uint64_t *claimed_sums, uint64_t *rounds,
                                                  uint64_t *points, uint64_t *factor_evals, uint64_t *final_evals,
                                                  size_t *bad_index);
/* host tables (canonical u64, ZIGZ_ERR_NOT_CANONICAL with the instance's index otherwise), narrowed and uploaded in one copy */
zigz_status zigz_sumcheck_prove_product_batch(zigz_ctx *ctx, size_t k, const unsigned *degrees,
                                              const uint64_t *const *factors, const size_t *ns,
                                              const uint64_t *fixed_challenges, uint64_t *claimed_sums, uint64_t *rounds,
                                              uint64_t *points, uint64_t *factor_evals, uint64_t *final_evals,
                                              size_t *bad_index);

/* k eq tables in ONE launch: table i has ns[i] = 2^v_i canonical words
 *   E_i[x] = prod_{j < v_i} (bit j of x ? tau_j : 1 - tau_j),
 * tau the v_i coordinates at points + sum_{j<i} v_j (concatenated in table order).  point[0] goes with the LSB of the index,
 * Multilinear.eval's convention (multilinear.zig:110-144): sum_x E_i[x] T[x] == zigz_dev_mle_eval(T, ns[i], tau, v_i) exactly, and
 * ns[i] == 1 gives the one-word table {1}.  With E_tau as the first factor, zigz_dev_sumcheck_prove_product_batch proves the
 * zero-check sum_x eq(tau, x) C(x) = 0 of a constraint C that is a product of up to two tables (the degree-3 rounds of
 * src/prover/prover.zig:237-288), and zigz_dev_sumcheck_verify_product_batch verifies it without the table.
 * d_out[i]: ns[i] packed u32 words of device memory, 16-byte aligned; nothing behind them is written.  Schedule: one small copy
 * (descriptors and factor pairs) and one launch for all k tables, queued on the context's stream; the call does not wait for
 * them -- the caller's next launch on the same stream sees the tables.
 * Every argument is checked for every table before anything is launched or written; the first failing table's index goes to
 * *bad_index (if non-NULL): ZIGZ_ERR_INVALID_ARGUMENT for ctx, ns, points or d_out NULL, k > ZIGZ_BATCH_MAX, an output that is
 * NULL or not 16-byte aligned, ns[i] > 2^32, or tables that together make 2^24 chunks of 8192 words or more (one launch's grid);
 * ZIGZ_ERR_EMPTY_EVALUATIONS / ZIGZ_ERR_LENGTH_NOT_POWER_OF_TWO for the length; ZIGZ_ERR_NOT_CANONICAL for a coordinate >= p.
 * k == 0 returns ZIGZ_OK and touches nothing.  Leaves the hint options, zigz_kernel_stats, an active commit job and open
 * zigz_merkle_batch handles alone. */
zigz_status zigz_dev_eq_table_batch(zigz_ctx *ctx, size_t k, const size_t *ns, const uint64_t *points, uint32_t *const *d_out,
                                    size_t *bad_index);
/* the same into host arrays of ns[i] canonical u64 words: built on the device, downloaded through pinned memory in chunks of at
 * most 32 MiB and widened on the way; returns when out is written */
zigz_status zigz_eq_table_batch(zigz_ctx *ctx, size_t k, const size_t *ns, const uint64_t *points, uint64_t *const *out,
                                size_t *bad_index);

/* k independent verifications of the proofs zigz_dev_sumcheck_prove_product_batch writes: SumcheckVerifier.verify
 * (src/proofs/sumcheck_verifier.zig:48-108, verifyRounds :172-205) with d + 1 coefficients per round, the oracle being the
 * product of the proof's d factors.  Proof i, in the prover's layout: degrees[i] = d_i in 1..ZIGZ_PRODUCT_MAX_DEGREE, ns[i] =
 * 2^v_i, rounds ((d_i + 1) v_i words, c_0..c_d per round), points (v_i), factor_evals (d_i; the array may be NULL) and
 * final_evals[i], claimed_sums[i]; everything concatenated in proof order.
 * FACTORS.  d_factors holds sum d_i pointers, proof by proof; factor_kinds (sum d_i bytes, or NULL: all tables) says what each
 * is: ZIGZ_FACTOR_TABLE -- the table at d_factors (ns[i] packed u32 words, 16-byte aligned); ZIGZ_FACTOR_EQ -- eq(tau, .), the
 * table zigz_dev_eq_table_batch would build, WITHOUT the table: its d_factors entry must be NULL and its tau is the next v_i words
 * of eq_points (the taus of all eq factors concatenated in factor order).
 * Per proof, bit for bit the reference: a fresh transcript, claim = claimed_sums[i]; per round reject if g(0) + g(1) != claim,
 * absorb c_0..c_d in order, draw the challenge (sumcheck_protocol.zig:176-184), claim = g(challenge).  Then every factor's
 * multilinear extension is evaluated at q -- the proof's point as given (flags == 0: the reference's behaviour, which REJECTS
 * honest proofs of two or more variables in general, see zigz_dev_sumcheck_verify_batch) or reversed
 * (ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED: where the prover's evaluations live) --: table factors in the batched eval's launch, one
 * (table, q) pair per factor, all proofs together; eq factors on the host in closed form, prod_j (tau_j q_j + (1 - tau_j)(1 -
 * q_j)).  The proof is accepted iff the rounds held, prod_j oracle_j == claim, prod_j oracle_j == final_evals[i] and, when
 * factor_evals != NULL, oracle_j == factor_evals[j] for every j.  (A zero-check's soundness also needs claimed_sums[i] == 0:
 * that comparison is the caller's.)
 * Outputs: verdicts[k] (may be NULL) 1 accept / 0 reject; *n_rejected; expected_evals[k] (may be NULL) the claim at the failing
 * round, or the final claim; oracle_evals (sum d_i words, may be NULL) every factor's evaluation, written for every proof
 * including those whose rounds failed.  For d_i == 1, a table factor and factor_evals == NULL these are
 * zigz_dev_sumcheck_verify_batch's values.
 * Schedule: the evaluation of all table factors is queued first, the host replays the k transcripts and computes the eq
 * factors on its threads meanwhile, and combines after the hand-off; a call without a table factor launches nothing.
 * Statuses are for the shape of the arguments only, never for what a proof holds; everything is checked for every proof
 * before anything is launched or written, and the first failing proof's index goes to *bad_index (if non-NULL):
 * ZIGZ_ERR_INVALID_ARGUMENT for ctx or n_rejected NULL, an unknown flag, a NULL input array when k > 0 (factor_kinds, eq_points
 * and factor_evals excepted), k > ZIGZ_BATCH_MAX, a degree outside 1..ZIGZ_PRODUCT_MAX_DEGREE, an unknown kind, an eq factor
 * whose pointer is not NULL or that has no eq_points, a table factor that is NULL or not 16-byte aligned, ns[i] > 2^32, or table
 * factors that together make 2^24 chunks of 8192 elements or more; the prover's rules per table (ns[i] == 1 is
 * ZIGZ_ERR_NO_VARIABLES); ZIGZ_ERR_NOT_CANONICAL for any word of a proof or of a tau >= p.  k == 0: ZIGZ_OK, *n_rejected = 0,
 * nothing else touched.  Leaves alone what zigz_dev_mle_eval_batch leaves alone. */
#define ZIGZ_FACTOR_TABLE 0
#define ZIGZ_FACTOR_EQ 1
zigz_status zigz_dev_sumcheck_verify_product_batch(zigz_ctx *ctx, size_t k, const unsigned *degrees,
                                                   const uint32_t *const *d_factors, const uint8_t *factor_kinds,
                                                   const uint64_t *eq_points, const size_t *ns, const uint64_t *claimed_sums,
                                                   const uint64_t *rounds, const uint64_t *points, const uint64_t *factor_evals,
                                                   const uint64_t *final_evals, uint32_t flags, uint8_t *verdicts,
                                                   uint64_t *expected_evals, uint64_t *oracle_evals, size_t *n_rejected,
                                                   size_t *bad_index);
/* host tables (canonical u64, ZIGZ_ERR_NOT_CANONICAL with the proof's index otherwise), narrowed and uploaded in one copy */
zigz_status zigz_sumcheck_verify_product_batch(zigz_ctx *ctx, size_t k, const unsigned *degrees, const uint64_t *const *factors,
                                               const uint8_t *factor_kinds, const uint64_t *eq_points, const size_t *ns,
                                               const uint64_t *claimed_sums, const uint64_t *rounds, const uint64_t *points,
                                               const uint64_t *factor_evals, const uint64_t *final_evals, uint32_t flags,
                                               uint8_t *verdicts, uint64_t *expected_evals, uint64_t *oracle_evals,
                                               size_t *n_rejected, size_t *bad_index);

/* k independent sumchecks of a SUM OF PRODUCTS of multilinear tables in shared launches (a constraint system under one
 * transcript): instance i has a POOL of M_i = n_tables[i] tables (1..ZIGZ_SOP_MAX_TABLES) of ns[i] = 2^v_i elements each and
 * T_i = n_terms[i] TERMS (1..ZIGZ_SOP_MAX_TERMS); term t is a coefficient alpha_t (canonical, 0 allowed) times a product of
 * d_t in 1..ZIGZ_PRODUCT_MAX_DEGREE pool tables named by index -- an index may repeat within a term and across terms, and a pool
 * table that no term names is bound and reported like the others.  The instance proves
 *   S_i = sum_{x in {0,1}^v_i} sum_{t < T_i} alpha_t prod_{j < d_t} pool[idx(t, j)](x)
 * with round polynomials of D_i + 1 coefficients c_0..c_D, D_i = max_t d_t (C(x) = sum_j alpha_j constraint_j(x),
 * src/prover/prover.zig:241-248).  Everything else is zigz_dev_sumcheck_prove_product_batch's: partialEval's MSB-first bind, a
 * fresh transcript per instance that absorbs c_0..c_D and then draws, fixed_challenges != NULL as the proveInteractive form, the
 * instances longer than 1024 on the device and the tails on the host after one hand-off.  With eq(tau, .) from
 * zigz_dev_eq_table_batch as a pool table that every term names this is the zero-check sum_x eq(tau, x) C(x) = 0 of a constraint
 * system C: one transcript, one point, every distinct table bound once per round.
 * Layout, everything concatenated in instance order: d_tables (sum M_i pointers), term_degrees and term_coeffs (sum T_i), term_tables
 * (one byte per factor, term by term: sum of all d_t).  Outputs: claimed_sums[k], rounds ((D_i + 1) v_i words), points (v_i),
 * table_evals (M_i: every pool table fully bound, i.e. its extension at the reversed point), final_evals[k] =
 * sum_t alpha_t prod_j table_evals[idx(t, j)].  With one term, alpha = 1 and distinct tables these are the product entry's words.
 * Schedule: per round one small copy, one data pass that loads, binds and stores every pool table of every live instance once and
 * multiplies out all terms, and one small finish launch; the workspace is 2 M_i ns[i] bytes per live instance.  The caller's
 * tables are only read.
 * Every argument is checked for every instance before anything is launched or written; the first failing instance's index goes to
 * *bad_index (if non-NULL): ZIGZ_ERR_INVALID_ARGUMENT for ctx or an array NULL (fixed_challenges excepted), k > ZIGZ_BATCH_MAX, M_i
 * or T_i outside 1..8, a term degree outside 1..ZIGZ_PRODUCT_MAX_DEGREE, a pool index >= M_i, a table that is NULL or not 16-byte
 * aligned, ns[i] > 2^ZIGZ_PRODUCT_MAX_LOG2_N, live instances that together make 2^24 chunks of 8192 elements or more;
 * ZIGZ_ERR_NO_VARIABLES for ns[i] == 1; ZIGZ_ERR_LENGTH_NOT_POWER_OF_TWO; ZIGZ_ERR_NOT_CANONICAL for a coefficient or a fixed
 * challenge >= p.  k == 0 returns ZIGZ_OK and touches nothing.  Leaves alone what the product entry leaves alone. */
#define ZIGZ_SOP_MAX_TABLES 8
#define ZIGZ_SOP_MAX_TERMS 8
zigz_status zigz_dev_sumcheck_prove_sop_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint32_t *const *d_tables,
                                              const size_t *ns, const unsigned *n_terms, const unsigned *term_degrees,
                                              const uint8_t *term_tables, const uint64_t *term_coeffs,
                                              const uint64_t *fixed_challenges, uint64_t *claimed_sums, uint64_t *rounds,
                                              uint64_t *points, uint64_t *table_evals, uint64_t *final_evals, size_t *bad_index);
/* host tables (canonical u64, ZIGZ_ERR_NOT_CANONICAL with the instance's index otherwise), narrowed and uploaded in one copy */
zigz_status zigz_sumcheck_prove_sop_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint64_t *const *tables,
                                          const size_t *ns, const unsigned *n_terms, const unsigned *term_degrees,
                                          const uint8_t *term_tables, const uint64_t *term_coeffs, const uint64_t *fixed_challenges,
                                          uint64_t *claimed_sums, uint64_t *rounds, uint64_t *points, uint64_t *table_evals,
                                          uint64_t *final_evals, size_t *bad_index);

/* k independent verifications of the proofs zigz_dev_sumcheck_prove_sop_batch writes, as zigz_dev_sumcheck_verify_product_batch
 * verifies a product proof: the prover's layout, and per POOL ENTRY table_kinds (sum M_i bytes, or NULL: all tables) --
 * ZIGZ_FACTOR_TABLE, the table at d_tables, or ZIGZ_FACTOR_EQ, eq(tau, .) without the table: its d_tables entry must be NULL and its
 * tau is the next v_i words of eq_points.  Per proof: the rounds are replayed with D_i + 1 coefficients (a fresh transcript,
 * claim = claimed_sums[i], reject if g(0) + g(1) != claim, absorb, draw, claim = g(challenge)); every table entry of the pool is
 * evaluated ONCE at q -- the proof's point as given (flags == 0) or reversed (ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED: where the prover's
 * evaluations live) -- in the batched eval's launch, one (table, q) pair per pool entry, all proofs together; eq entries on the
 * host in closed form; the oracle is sum_t alpha_t prod_j oracle[idx(t, j)].  The proof is accepted iff the rounds held, the oracle
 * equals the last claim and final_evals[i] and, when table_evals != NULL, every entry's oracle equals its table eval.  (A
 * zero-check's soundness also needs claimed_sums[i] == 0: that comparison is the caller's.)
 * Outputs: verdicts[k] (may be NULL) 1 accept / 0 reject; *n_rejected; expected_evals[k] (may be NULL) the claim at the failing
 * round, or the final claim; oracle_evals (sum M_i words, may be NULL) every pool entry's evaluation, written for every proof
 * including the rejected ones.  A call without a table entry launches nothing.
 * Statuses are for the shape of the arguments only; everything is checked for every proof before anything is launched or
 * written, and the first failing proof's index goes to *bad_index (if non-NULL): ZIGZ_ERR_INVALID_ARGUMENT for ctx or n_rejected
 * NULL, an unknown flag, a NULL input array when k > 0 (table_kinds, eq_points and table_evals excepted), k > ZIGZ_BATCH_MAX, M_i or
 * T_i outside 1..8, a term degree outside 1..ZIGZ_PRODUCT_MAX_DEGREE, a pool index >= M_i, an unknown kind, an eq entry whose pointer
 * is not NULL or that has no eq_points, a table entry that is NULL or not 16-byte aligned, ns[i] > 2^32, or table entries that
 * together make 2^24 chunks of 8192 elements or more; the prover's rules per table (ns[i] == 1 is ZIGZ_ERR_NO_VARIABLES);
 * ZIGZ_ERR_NOT_CANONICAL for any word of a proof, a coefficient or a tau >= p.  k == 0: ZIGZ_OK, *n_rejected = 0, nothing else
 * touched. */
zigz_status zigz_dev_sumcheck_verify_sop_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint32_t *const *d_tables,
                                               const uint8_t *table_kinds, const uint64_t *eq_points, const size_t *ns,
                                               const unsigned *n_terms, const unsigned *term_degrees, const uint8_t *term_tables,
                                               const uint64_t *term_coeffs, const uint64_t *claimed_sums, const uint64_t *rounds,
                                               const uint64_t *points, const uint64_t *table_evals, const uint64_t *final_evals,
                                               uint32_t flags, uint8_t *verdicts, uint64_t *expected_evals, uint64_t *oracle_evals,
                                               size_t *n_rejected, size_t *bad_index);
/* host tables (canonical u64, ZIGZ_ERR_NOT_CANONICAL with the proof's index otherwise), narrowed and uploaded in one copy */
zigz_status zigz_sumcheck_verify_sop_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint64_t *const *tables,
                                           const uint8_t *table_kinds, const uint64_t *eq_points, const size_t *ns,
                                           const unsigned *n_terms, const unsigned *term_degrees, const uint8_t *term_tables,
                                           const uint64_t *term_coeffs, const uint64_t *claimed_sums, const uint64_t *rounds,
                                           const uint64_t *points, const uint64_t *table_evals, const uint64_t *final_evals,
                                           uint32_t flags, uint8_t *verdicts, uint64_t *expected_evals, uint64_t *oracle_evals,
                                           size_t *n_rejected, size_t *bad_index);

/* k independent ZERO-CHECK sumchecks with the eq factor in closed form: instance i proves
 *   S_i = sum_{x in {0,1}^v_i} eq(tau_i, x) C_i(x),   C_i(x) = sum_{t < T_i} alpha_t prod_{j < d_t} pool[idx(t, j)](x),
 * over zigz_dev_sumcheck_prove_sop_batch's pool of M_i tables (1..8, NONE of them eq) and T_i terms (1..8) of degree d_t in
 * 1..ZIGZ_PRODUCT_MAX_DEGREE, with the same layout, index and coefficient rules.  tau_i is the next v_i canonical words of eq_points,
 * tau[0] going with the LSB of x as in zigz_dev_eq_table_batch.  No eq table is built, bound or stored: round r binds index bit
 * v - 1 - r (the MSB-first bind), so the weight factors as s_r(X) = P_r ((1 - tau_j) + (2 tau_j - 1) X) t_r(X) with j = v - 1 - r,
 * P_r the product of eq(tau_{v-1-r'}, challenge_r') over the rounds so far, and t_r the round polynomial of C weighted pair by pair
 * with the eq table of the PREFIX tau_0..tau_{v-r-2}, which the passes form from two small tables.  The proof is word for word the
 * one the sop entry writes with the materialised eq table appended to the pool and named by every term -- but C may have degree 3:
 * a round has D_i + 2 coefficients c_0..c_{D+1}, D_i = max_t d_t, at most ZIGZ_ZEROCHECK_MAX_DEGREE + 1.  A fresh transcript per
 * instance absorbs all D_i + 2 coefficients in order and then draws; fixed_challenges != NULL as there.
 * Outputs: claimed_sums[k], rounds ((D_i + 2) v_i words), points (v_i), table_evals (M_i: every pool table fully bound, i.e. at
 * the reversed point), eq_evals[k] = eq(tau_i, .) at the reversed point, final_evals[k] = eq_evals[i] * sum_t alpha_t prod_j
 * table_evals[idx(t, j)].  Schedule and limits are the sop entry's (instances longer than 1024 on the device, one small copy, one
 * data pass and one finish launch per round, the tails on the host after one hand-off; the weights travel with the first copy);
 * the workspace is 2 M_i ns[i] bytes per live instance.  The caller's tables are only read.
 * Every argument is checked for every instance before anything is launched or written, with the sop entry's statuses in its order
 * (eq_points and eq_evals must not be NULL); then, per instance, ZIGZ_ERR_NOT_CANONICAL for a tau word >= p.  k == 0 returns
 * ZIGZ_OK and touches nothing. */
#define ZIGZ_ZEROCHECK_MAX_DEGREE 4
zigz_status zigz_dev_sumcheck_prove_zerocheck_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint32_t *const *d_tables,
                                                    const size_t *ns, const unsigned *n_terms, const unsigned *term_degrees,
                                                    const uint8_t *term_tables, const uint64_t *term_coeffs, const uint64_t *eq_points,
                                                    const uint64_t *fixed_challenges, uint64_t *claimed_sums, uint64_t *rounds,
                                                    uint64_t *points, uint64_t *table_evals, uint64_t *eq_evals, uint64_t *final_evals,
                                                    size_t *bad_index);
/* host tables (canonical u64, ZIGZ_ERR_NOT_CANONICAL with the instance's index otherwise), narrowed and uploaded in one copy */
zigz_status zigz_sumcheck_prove_zerocheck_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint64_t *const *tables,
                                                const size_t *ns, const unsigned *n_terms, const unsigned *term_degrees,
                                                const uint8_t *term_tables, const uint64_t *term_coeffs, const uint64_t *eq_points,
                                                const uint64_t *fixed_challenges, uint64_t *claimed_sums, uint64_t *rounds,
                                                uint64_t *points, uint64_t *table_evals, uint64_t *eq_evals, uint64_t *final_evals,
                                                size_t *bad_index);

/* k independent verifications of the proofs zigz_dev_sumcheck_prove_zerocheck_batch writes, as zigz_dev_sumcheck_verify_sop_batch
 * verifies a sop proof: the prover's layout and eq_points.  Per proof: the rounds are replayed with D_i + 2 coefficients (a fresh
 * transcript, claim = claimed_sums[i], reject if g(0) + g(1) != claim, absorb, draw, claim = g(challenge)); every pool table is
 * evaluated ONCE at q -- the proof's point as given (flags == 0) or reversed (ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED: where the
 * prover's evaluations live) -- in the batched eval's launch; eq(tau_i, q) on the host in closed form; the oracle is eq(tau_i, q) *
 * sum_t alpha_t prod_j oracle[idx(t, j)].  The proof is accepted iff the rounds held, the oracle equals the last claim and
 * final_evals[i], and every given eval (table_evals, eq_evals: each may be NULL) equals its oracle.  (A zero-check's soundness also
 * needs claimed_sums[i] == 0: that comparison is the caller's.)
 * Outputs: verdicts[k] (may be NULL); *n_rejected; expected_evals[k] (may be NULL) the claim at the failing round, or the final
 * claim; oracle_evals (sum M_i words, may be NULL) every pool table's evaluation, written for every proof.  A call with no
 * instances launches nothing.
 * Statuses are for the shape of the arguments only, checked for every proof before anything is launched or written; the first
 * failing proof's index goes to *bad_index (if non-NULL): ZIGZ_ERR_INVALID_ARGUMENT for ctx or n_rejected NULL, an unknown flag, a
 * NULL input array when k > 0 (table_evals and eq_evals excepted), k > ZIGZ_BATCH_MAX, M_i or T_i outside 1..8, a term degree
 * outside 1..ZIGZ_PRODUCT_MAX_DEGREE, a pool index >= M_i, a table that is NULL or not 16-byte aligned, ns[i] > 2^32, or tables that
 * together make 2^24 chunks of 8192 elements or more; the prover's rules per table (ns[i] == 1 is ZIGZ_ERR_NO_VARIABLES);
 * ZIGZ_ERR_NOT_CANONICAL for any word of a proof, a coefficient or a tau >= p.  k == 0: ZIGZ_OK, *n_rejected = 0, nothing else
 * touched. */
zigz_status zigz_dev_sumcheck_verify_zerocheck_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint32_t *const *d_tables,
                                                     const uint64_t *eq_points, const size_t *ns, const unsigned *n_terms,
                                                     const unsigned *term_degrees, const uint8_t *term_tables,
                                                     const uint64_t *term_coeffs, const uint64_t *claimed_sums, const uint64_t *rounds,
                                                     const uint64_t *points, const uint64_t *table_evals, const uint64_t *eq_evals,
                                                     const uint64_t *final_evals, uint32_t flags, uint8_t *verdicts,
                                                     uint64_t *expected_evals, uint64_t *oracle_evals, size_t *n_rejected,
                                                     size_t *bad_index);
/* host tables (canonical u64, ZIGZ_ERR_NOT_CANONICAL with the proof's index otherwise), narrowed and uploaded in one copy */
zigz_status zigz_sumcheck_verify_zerocheck_batch(zigz_ctx *ctx, size_t k, const unsigned *n_tables, const uint64_t *const *tables,
                                                 const uint64_t *eq_points, const size_t *ns, const unsigned *n_terms,
                                                 const unsigned *term_degrees, const uint8_t *term_tables, const uint64_t *term_coeffs,
                                                 const uint64_t *claimed_sums, const uint64_t *rounds, const uint64_t *points,
                                                 const uint64_t *table_evals, const uint64_t *eq_evals, const uint64_t *final_evals,
                                                 uint32_t flags, uint8_t *verdicts, uint64_t *expected_evals, uint64_t *oracle_evals,
                                                 size_t *n_rejected, size_t *bad_index);

/* k independent PRODUCT TREES: column i holds n = ns[i] = 2^v canonical words, V_v = column, V_j[x] = V_{j+1}[x] * V_{j+1}[x + 2^j]
 * for x < 2^j (the HALVES pairing: it matches the MSB-first bind of the sumchecks, and the two operands of a layer are contiguous
 * sub-arrays), down to V_0[0] = the product of all n words.  d_out[i]: ns[i] packed u32 words, 16-byte aligned; layer j (2^j
 * canonical words) sits at word ns[i] - 2^(j+1) for j = v - 1 .. 0, so every layer of 4 words or more is 16-byte aligned and the
 * product is word ns[i] - 2; word ns[i] - 1 is not written and nothing behind the buffer is.  The layers above 2048 words are
 * computed by passes of up to three fused levels, one launch per pass for all columns (about 4 n bytes read and 3.5 n written
 * per pass); the rest by one workgroup per column.  The call is queued on the context's stream and does not wait, like
 * zigz_dev_eq_table_batch.  The columns are only read (and not checked: a word >= p gives an unspecified canonical product).
 * Every argument is checked for every column before anything is launched or written; the first failing column's index goes to
 * *bad_index (if non-NULL): ZIGZ_ERR_INVALID_ARGUMENT for ctx or an array NULL, k > ZIGZ_BATCH_MAX, a column or output that is
 * NULL or not 16-byte aligned, ns[i] > 2^ZIGZ_PRODUCT_MAX_LOG2_N, columns longer than 2048 that together make 2^24 chunks of 8192
 * words or more; ZIGZ_ERR_EMPTY_EVALUATIONS / ZIGZ_ERR_LENGTH_NOT_POWER_OF_TWO for the shape; ZIGZ_ERR_NO_VARIABLES for
 * ns[i] == 1.  k == 0 returns ZIGZ_OK and touches nothing. */
zigz_status zigz_dev_product_layers_batch(zigz_ctx *ctx, size_t k, const uint32_t *const *d_tables, const size_t *ns,
                                          uint32_t *const *d_out, size_t *bad_index);
/* host columns (canonical u64, ZIGZ_ERR_NOT_CANONICAL with the column's index otherwise), narrowed and uploaded in one copy;
 * out[i]: ns[i] u64 words in the same layout (word ns[i] - 1 is not written).  Waits for the trees. */
zigz_status zigz_product_layers_batch(zigz_ctx *ctx, size_t k, const uint64_t *const *tables, const size_t *ns, uint64_t *const *out,
                                      size_t *bad_index);

/* k independent GRAND-PRODUCT arguments (the layered, GKR-style product tree): instance i proves that products[i] is the product
 * of the n = ns[i] = 2^v words of its column A.  With the tree above, L_j = V_{j+1}[0 : 2^j] and H_j = V_{j+1}[2^j : 2^(j+1)].
 * Points are in Multilinear.eval's convention throughout (coordinate 0 goes with the LSB of the index).  Per instance ONE
 * transcript, fresh at the start, used in this order:
 *   1. absorb products[i];
 *   2. layer 0: l_0 = V_1[0], h_0 = V_1[1]; absorb l_0, h_0; draw c_0; tau^(1) = (c_0), claim_1 = l_0 + c_0 (h_0 - l_0);
 *   3. layer j = 1 .. v - 1: the closed-form zero-check (zigz_dev_sumcheck_prove_zerocheck_batch with the pool (L_j, H_j), the
 *      one term L_j * H_j and tau^(j)) of sum_x eq(tau^(j), x) L_j(x) H_j(x) = claim_j: j rounds of 4 coefficients, each absorbed
 *      and then drawn from as there; with q the round challenges reversed, l_j = L_j(q), h_j = H_j(q); absorb l_j, h_j; draw c_j;
 *      tau^(j+1) = (q_0, .., q_{j-1}, c_j), claim_(j+1) = l_j + c_j (h_j - l_j);
 *   4. leaf_point = tau^(v), leaf_eval = claim_v, which equals A(leaf_point) for an honest prover.
 * Outputs, concatenated in instance order: products (1 word per instance), layer_evals (2 v: l_j, h_j for j = 0 .. v - 1), rounds
 * (2 v (v - 1): layer by layer, each round c_0..c_3), points (v (v - 1) / 2: layer by layer, in round order), layer_challenges
 * (v), leaf_points (v), leaf_evals (1).  fixed_challenges != NULL is the interactive form: v (v + 1) / 2 words per instance in
 * order of use (c_0, layer 1's round challenge, c_1, layer 2's two, c_2, ...), no transcript.
 * Schedule: the trees of all instances are built into a workspace (ns[i] words each; the leaf layer is the caller's column, which
 * is only read) and the top of every tree -- the layers of at most 2048 words -- is handed to the host ONCE; the host runs layer
 * 0 and the layers whose tables are at most 1024 long for all instances in parallel; then, for j = 11 .. max v - 1, ONE run of
 * the zero-check schedule serves layer j of every instance with v_i > j.
 * Every argument is checked for every instance before anything is launched or written, with zigz_dev_product_layers_batch's
 * statuses in its order; then, per instance, ZIGZ_ERR_NOT_CANONICAL for a fixed challenge >= p; an output array NULL is
 * ZIGZ_ERR_INVALID_ARGUMENT.  The column on the device is not checked on the way in; a value >= p that reaches the host is
 * ZIGZ_ERR_NOT_CANONICAL.  k == 0 returns ZIGZ_OK and touches nothing. */
zigz_status zigz_dev_grand_product_prove_batch(zigz_ctx *ctx, size_t k, const uint32_t *const *d_tables, const size_t *ns,
                                               const uint64_t *fixed_challenges, uint64_t *products, uint64_t *layer_evals,
                                               uint64_t *rounds, uint64_t *points, uint64_t *layer_challenges, uint64_t *leaf_points,
                                               uint64_t *leaf_evals, size_t *bad_index);
/* host columns (canonical u64, ZIGZ_ERR_NOT_CANONICAL with the instance's index otherwise), narrowed and uploaded in one copy */
zigz_status zigz_grand_product_prove_batch(zigz_ctx *ctx, size_t k, const uint64_t *const *tables, const size_t *ns,
                                           const uint64_t *fixed_challenges, uint64_t *products, uint64_t *layer_evals, uint64_t *rounds,
                                           uint64_t *points, uint64_t *layer_challenges, uint64_t *leaf_points, uint64_t *leaf_evals,
                                           size_t *bad_index);

/* k independent verifications of the Fiat-Shamir proofs zigz_dev_grand_product_prove_batch writes, in its layout.  Every
 * challenge is derived here, from one transcript per proof: l_0 h_0 == products[i]; per layer j >= 1 the claim chain (g(0) +
 * g(1) == claim, absorb, draw, claim = g(challenge)) and eq(tau^(j), q) l_j h_j == the last claim; the derived leaf point must
 * equal leaf_points, leaf_evals[i] must equal claim_v, and so must the column's evaluation A(leaf_points[i]) -- queued for all
 * proofs in the batched eval's launch FIRST, while the host's threads replay the layers.
 * ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED is for a caller that holds a commitment, not the column: d_tables must be NULL, nothing is
 * launched, and a proof is accepted iff the layers hold, the leaf point is the derived one and leaf_evals[i] == claim_v;
 * A(leaf_point) == leaf_evals[i] is then the CALLER'S check, for example through zigz_commit_open.
 * Outputs: verdicts[k] (may be NULL); *n_rejected; expected_evals[k] (may be NULL) the claim at the failing step -- the product
 * check, a round, a layer's final check -- or claim_v; oracle_evals[k] (may be NULL; not written with the flag) the column's
 * evaluation at leaf_points[i].
 * Statuses are for the shape of the arguments only, checked for every proof before anything is launched or written; the first
 * failing proof's index goes to *bad_index (if non-NULL): ZIGZ_ERR_INVALID_ARGUMENT for ctx or n_rejected NULL, an unknown flag, a
 * NULL input array when k > 0, columns given with the flag or missing without it, k > ZIGZ_BATCH_MAX, a column that is NULL or not
 * 16-byte aligned, ns[i] > 2^ZIGZ_PRODUCT_MAX_LOG2_N; the prover's rules for the shape (ns[i] == 1 is ZIGZ_ERR_NO_VARIABLES);
 * ZIGZ_ERR_NOT_CANONICAL for any word of a proof >= p.  k == 0: ZIGZ_OK, *n_rejected = 0, nothing else touched. */
#define ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED 1u
zigz_status zigz_dev_grand_product_verify_batch(zigz_ctx *ctx, size_t k, const uint32_t *const *d_tables, const size_t *ns,
                                                const uint64_t *products, const uint64_t *layer_evals, const uint64_t *rounds,
                                                const uint64_t *leaf_points, const uint64_t *leaf_evals, uint32_t flags,
                                                uint8_t *verdicts, uint64_t *expected_evals, uint64_t *oracle_evals, size_t *n_rejected,
                                                size_t *bad_index);
/* host columns (canonical u64, ZIGZ_ERR_NOT_CANONICAL with the proof's index otherwise), narrowed and uploaded in one copy */
zigz_status zigz_grand_product_verify_batch(zigz_ctx *ctx, size_t k, const uint64_t *const *tables, const size_t *ns,
                                            const uint64_t *products, const uint64_t *layer_evals, const uint64_t *rounds,
                                            const uint64_t *leaf_points, const uint64_t *leaf_evals, uint32_t flags, uint8_t *verdicts,
                                            uint64_t *expected_evals, uint64_t *oracle_evals, size_t *n_rejected, size_t *bad_index);

/* ---------------------------------------------------------------- host SHA3 sponge / transcript
 * FiatShamirTranscript   src/core/hash.zig:255-324 (sequential by construction: stays on the host) */
zigz_transcript *zigz_transcript_new(void);
void zigz_transcript_free(zigz_transcript *t);
void zigz_transcript_append_bytes(zigz_transcript *t, const uint8_t *data, size_t len);
void zigz_transcript_append_field(zigz_transcript *t, uint64_t canonical_value);
/* appends `count` times:  tag bytes then LE64((start + k) mod p), k = 0..count-1
 * (the "LASSO_TABLE" loop of prover.zig:302-312 in one call) */
void zigz_transcript_append_tagged_counter(zigz_transcript *t, const uint8_t *tag, size_t tag_len,
                                           uint64_t start, uint64_t count);
uint64_t zigz_transcript_challenge(zigz_transcript *t); /* BabyBear; hash.zig:301-316 */
void zigz_sha3_256(const uint8_t *data, size_t len, uint8_t out[32]);
void zigz_sha256(const uint8_t *data, size_t len, uint8_t out[32]);
/* which single-state Keccak-f[1600] the host sponge uses ("scalar", "bmi2", "avx512f" or "avx512vl": the fastest
 * supported variant, timed at load; env ZIGZ_HOST_KECCAK overrides), and one permutation through a chosen variant
 * (0 = the picked one, 1 = scalar, 2 = bmi2, 3 = avx512f, 4 = avx512vl) -- diagnostics / self-test */
const char *zigz_host_keccak_impl(void);
void zigz_host_keccak_permute(uint64_t state[25], int which);
/* Sponge service for a host that proves several traces at once (one thread per proof).  A proof's transcript is a chain of
 * ~147 k dependent permutations at a 2^20 trace (prover.zig:302-312) and one permutation costs the same ~880 cycles whether
 * its lanes sit in xmm or zmm registers, so `n` server threads each advance up to 8 transcripts' tagged-counter absorptions
 * in lock step -- one 8-way AVX-512 permutation per block -- while the proofs' own threads sleep.  Same bytes absorbed, same
 * challenges.  n = 0 (default): every transcript absorbs on its own thread.  Ignored without AVX-512F.  Call while no
 * transcript is absorbing.  zigz_host_keccak_permute_x8: the 8-way permutation on states[lane][slot] (25 x 8 u64, 64-byte
 * aligned) -- diagnostics / self-test, requires AVX-512F. */
void zigz_host_sponge_servers(int n);
int zigz_host_sponge_batching(void);
void zigz_host_keccak_permute_x8(uint64_t *states);

/* ---------------------------------------------------------------- measurement hooks (bench.py)
 * Average device time (microseconds, HIP events on the context's stream) of the last call's
 * dominant kernels; reset by each API call that records them. */
typedef struct zigz_kernel_stats {
    double merkle_build_us;   /* all Keccak leaf + level launches of the last commit_begin */
    double eval_us;           /* all MLE fold / eval launches of the last commit_open_all */
    double path_us;           /* path gather */
    double bind_us;           /* last zigz_dev_mle_bind / bind_sums launch, or all binds of the last sumcheck */
    uint64_t bind_launches;
    uint64_t keccak_permutations; /* Keccak-f[1600] actually computed by the last commit (table look-ups and chained uniform blocks excluded) */
    /* the bulk MLE-bind launches of the last eval / sumcheck / bind call, each timed on its own: total device time,
     * launch count, algorithmic bytes.  Kernel k_radix_fold (one pass binding v-10 variables, 4 B read per element;
     * timed with the dispatch's own begin/end timestamps) for evals of tables >= 2^14, k_bind_vec (6 B per table
     * element; HIP event pair around the launch) otherwise. */
    double bind_vec_us;
    uint64_t bind_vec_launches;
    uint64_t bind_vec_bytes;
    /* run-aware Merkle levels (option "run_aware_mask") of the last batched commit: columns built that way, the nodes
     * of the levels they covered (levels 0 .. v - 8: what a dense build hashes there), how many of those were hashed rather
     * than copied from the left neighbour, and the kernel time of the structure + hashing launches (timing mode).  0 when the
     * option is off or the trees have fewer than 2^15 leaves. */
    uint64_t run_aware_columns;
    uint64_t run_aware_dense_nodes;
    uint64_t run_aware_hashed;
    double run_aware_us;
    /* content-addressed levels (option "cons_group_mask") of the last batched commit: columns of the group, the nodes of the
     * levels they covered (what a dense build hashes there) and the digests actually computed (representatives x columns) */
    uint64_t cons_columns;
    uint64_t cons_dense_nodes;
    uint64_t cons_hashed;
    uint64_t cons_probe_distinct; /* distinct leaves (tuples) of the group; > 1/4 of the leaves: dropped, cons_columns = 0 (0 when the group was not tried) */
    /* Keccak launches of the last batched commit by class, each launch timed with its own begin / end timestamps
     * (kernel time as rocprofv3 --kernel-trace reports it; the gaps between launches are in merkle_build_us only):
     * k_keccak_leaves; k_keccak_level<4> (the large levels); k_keccak_level<1> (the small levels); hashes = permutations */
    double keccak_leaves_us;
    uint64_t keccak_leaves_perms;
    double keccak_level_wide_us;
    uint64_t keccak_level_wide_perms;
    double keccak_level_small_us;
    uint64_t keccak_level_small_perms;
    /* option "small_domain_mask": columns whose levels 0-1 came from the constant tables in the last batched commit, the
     * kernel time of that launch, and the number of waves that found a value >= 128 and hashed instead */
    uint64_t small_domain_columns;
    double small_domain_us;
    uint64_t small_domain_fallback_waves;
    /* the structure-aware build of the last batched commit (timing mode), by class: structure_us = the passes that decide
     * WHICH nodes are hashed (run-aware stages k_runs_stage, content-addressing table passes k_cons_*: no hashing);
     * list_hash_us / list_hash_perms = the per-level launches that hash those lists (k_level_hash) and the permutations they
     * computed; top_us / top_perms = the last 8 levels (k_merkle_top).  run_aware_us = structure_us + list_hash_us. */
    double structure_us;
    double list_hash_us;
    uint64_t list_hash_perms;
    double top_us;
    uint64_t top_perms;
    /* builds that zigz_commit_roots had to repeat on this context because a list of the structure-aware levels ran out of the
     * room learnt from earlier builds (or the group was dropped and its columns had no slabs): a running count */
    uint64_t rebuilds;
    /* hinted (run-aware) columns of the last commit job whose N values are all equal -- established from the values by the
     * structure pass -- and which zigz_commit_open_all therefore did not read again: the multilinear extension of a constant is
     * that constant */
    uint64_t eval_constant_columns;
} zigz_kernel_stats;
/* One hot kernel, `iters` (<= 64) launches on a synthetic device-resident table of ncols columns x 2^nv elements, each
 * launch timed by its own begin / end timestamps.  kernel: "k_bind_vec" (partialEval, multilinear.zig:154-180, 6 B per
 * table element), "k_bind_vec_sums" (the same fused with the next roundPolynomial), "k_half_sums" / "k_block_sums"
 * (roundPolynomial / sumOverHypercube, multilinear.zig:188-232: kernel k_block_sums with 2 resp. 1024 blocks, 4 B per
 * element; "k_block_sums": ncols = 1),
 * "k_radix_fold" (eval, multilinear.zig:110-144, 4 B per element + partial sums), "k_keccak_leaves" / "k_keccak_level"
 * (hash.zig:135-147,187-195; units = permutations), "k_lasso_fingerprints" (lasso_prover.zig:208-239; units = rows of 3
 * fields).  cold != 0: a 1 GiB read sweep before every launch empties L2 / Infinity Cache of the table. */
typedef struct zigz_bench_result {
    double avg_us, min_us, max_us;
    uint64_t algorithmic_bytes; /* per launch */
    uint64_t units;             /* table elements / permutations / rows per launch */
    uint32_t launches;
} zigz_bench_result;
zigz_status zigz_bench_kernel(zigz_ctx *ctx, const char *kernel, size_t nv, size_t ncols, int iters, int cold,
                              zigz_bench_result *out);
zigz_status zigz_ctx_enable_timing(zigz_ctx *ctx, int enable);
/* Timing mode, launch by launch: the timed launches of the context's last commit job (its build after zigz_commit_roots, its
 * eval fold after zigz_commit_open_all) with their own begin / end on ONE time axis -- microseconds since the epoch of
 * `zigz_ctx_set_epoch` -- so that a caller that runs many contexts at once can take the UNION of a kernel class's intervals
 * (time during which at least one launch of the class was on the GPU) instead of the sum of durations of launches that
 * overlap.  The events carry the dispatch's own timestamps (first wave started .. last wave ended: within 1 us of a clock
 * read inside the kernel, tools/event_semantics.hip; a launch's wait behind its predecessor in the stream is not part of it,
 * its wait for wave slots next to other streams' kernels is), and are comparable across the streams of a device.
 * zigz_ctx_set_epoch(ctx, owner): owner == ctx records a new epoch on the context's stream; otherwise ctx adopts the
 * owner's (which must outlive its use).  Without an epoch, times count from the job's first timed launch.
 * class: 0 k_keccak_leaves, 1 / 2 k_keccak_level (wide / small), 3 k_keccak_small_l01, 4 structure passes (k_runs_stage,
 * k_cons_*: first .. last launch of each group), 5 k_level_hash, 6 k_merkle_top, 7 k_radix_fold (eval). */
typedef struct zigz_launch_rec {
    uint32_t cls;
    uint32_t reserved;
    uint64_t perms;      /* Keccak permutations where the host knows them at launch time (classes 0-2, 6), else 0 */
    double start_us, end_us;
} zigz_launch_rec;
zigz_status zigz_ctx_set_epoch(zigz_ctx *ctx, zigz_ctx *owner);
zigz_status zigz_ctx_launch_log(zigz_ctx *ctx, zigz_launch_rec *out, size_t cap, size_t *n);
/* tuning / test switches: "per_round_sumcheck" = 1 forces the one-launch-per-round sumcheck form;
 * "fold_eval" = 1 forces eval by v successive binds instead of the one-pass radix form;
 * "run_aware_mask" = bit c set: column c of the following batched commits (<= 64 columns, 2^15 .. 2^26 rows) is expected to be
 *   piecewise constant -- in the witness of prover.zig:376-390 the registers: every RV64IM step writes at most one of them
 *   (state.zig writeReg), so the 31 columns x1..x31 together change at most once per step.  On the levels 0 .. v - 8 (down to
 *   256 nodes per column) a node whose subtree and its left neighbour's are uniform with the same value takes the
 *   neighbour's digest instead of being hashed.  Decided from the VALUES on the device, never from the hint: identical trees
 *   for ANY input; with c change points in a column a level costs <= min(nodes, 2 c + one per tile) hashes (a tile is what one
 *   4096-leaf segment covers at that level).
 *   In a commit job only the hashed nodes have a digest at all, stored in LIST ORDER; the next level's hashes and
 *   zigz_commit_open_all find a copy's digest through a per-level bitmap of hashed nodes.  The room for those lists is what the
 *   context's earlier jobs needed (+ 25 %), not the worst case: a job that runs out notices on the device and
 *   zigz_commit_roots repeats its build with more (kernel_stats.rebuilds) -- typically once, the first time a context meets
 *   a new kind of trace.  "run_aware_materialize" = 1 writes every digest of every tree into node-addressed trees (tests that
 *   compare whole trees); single trees (zigz_merkle_commit) always do.
 * "cons_group_mask" = bit c set: the columns of this set repeat in the same places -- in the witness of prover.zig:376-390
 *   the ten columns that are functions of the instruction at pc (pc, x0, opcode, rd, rs1, rs2, funct3, funct7, imm, is_read):
 *   wherever the program loops, the same nodes recur in all of them, at most P distinct ones per level for a loop of P steps.
 *   On the levels 0 .. v - 8 a device hash table finds for every node the first node of its level with the same content in
 *   ALL columns of the group (leaves: the tuple of values, fingerprinted and verified; above: the pair of the children's
 *   representatives -- the identity of the hash input itself), and only representatives are hashed, once per column.  Takes
 *   precedence over the two other hints; identical trees for ANY input; the other nodes are virtual like run-aware copies.
 *   A group that does not repeat -- more than a quarter of its leaves distinct -- is DROPPED: its columns are built like any
 *   others (the other hints then apply to them).  That decision is taken on the device after the leaf level's table pass and
 *   read by the later launches from device memory: zigz_commit_begin* never waits for it.  (The first job of a context that
 *   drops its group is built twice -- the columns had no node-addressed trees to be built into; a context whose last two
 *   jobs dropped the group does not try it in its next 15 jobs; "cons_always" = 1 tries in every job.)
 * "merkle_dedup" = 1 / 0 is shorthand for run_aware_mask = all ones / 0;
 * "small_domain_mask" = bit c set: column c of the following batched commits (<= 64 columns, >= 1024 rows) holds values
 *   < 128 BY CONSTRUCTION -- in the witness of prover.zig:376-390 that is x0 (always 0, registers.zig:38-48), the
 *   instruction fields opcode / rd / rs1 / rs2 / funct3 / funct7 (7-, 5-, 5-, 5-, 3-, 7-bit fields, rv64i.zig:124-151) and
 *   mem.is_read (0 / 1) -- so its leaf digests SHA3(LE64(v)) and level-1 nodes are looked up in two constant tables
 *   (128 + 128^2 digests) instead of hashed: 1.5 N of the 2 N permutations of such a column.  The bound is checked per
 *   wave on the device; where it does not hold the digests are hashed, so the trees are identical for ANY input. */
zigz_status zigz_ctx_set_option(zigz_ctx *ctx, const char *name, int64_t value);
/* the current value of an option (every name above except the shorthand "merkle_dedup"): lets a caller that changes the
 * hint masks for one proof put back what the context's owner had set (host/prover.cpp does) */
zigz_status zigz_ctx_get_option(zigz_ctx *ctx, const char *name, int64_t *value);
zigz_status zigz_ctx_get_stats(zigz_ctx *ctx, zigz_kernel_stats *out);

#ifdef __cplusplus
}
#endif
#endif
