// Host-side functions that cross the .hip files without being part of the C ABI (include/mmda_hip.h), each declared once, grouped by
// the file that defines it.  The fused row launches have a header of their own (fused_rows.h), the split-K reduce sits beside its job
// struct (splitk.h).
#pragma once
#include "common.h"

// ---- api.hip
void mmda_set_error(const char* what, hipError_t e);
#define MMDA_CHECK_LAUNCH(name)                                   \
  do {                                                            \
    hipError_t _e = hipGetLastError();                            \
    if (_e != hipSuccess) { mmda_set_error(name, _e); return MMDA_ELAUNCH; } \
  } while (0)
float* mmda_scratch_get(hipStream_t s, size_t bytes);       // per-stream scratch: valid until the stream's next request

// ---- gemm.hip: mmda_gemm_grouped with split-K sized as if `absent` were launched too
int mmda_gemm_grouped_sized(const mmda_gemm_args* args, int n, const mmda_gemm_args* absent, int n_absent, void* stream);

// ---- norm.hip
// the backward of up to four plain LayerNorms in the 16-byte form, gamma / beta gradients left as per-block partials in `parts`
bool mmda_ln_bwd_parts_applies(const mmda_ln_bwd_args* a, int n);
int64_t mmda_ln_parts_floats(const mmda_ln_bwd_args* a, int n);
int mmda_ln_bwd_parts(const mmda_ln_bwd_args* a, int n, float* parts, void* stream);
int mmda_ln_parts_finish(const mmda_ln_bwd_args* a, int n, float* parts, void* stream);

// ---- embed_rows.hip: lists of (id, row) pairs into rows of the embedding table
// What describes a list: n positions p = t * B + b with ids[p] and the D floats rows[p]; `sorted` (optional): the list as
// mmda_embed_sort_ids left it; lengths / B (optional): position p is padding, and skipped, when t >= lengths[b].  The list's length and
// `sorted` decide the form the sums take, inside embed_rows.hip and nowhere else.
struct EmbedList { const int64_t* ids; const unsigned* sorted; int n, D; const float* rows; const int* lengths; int B; };
bool mmda_embed_scatter_sorts(int rows);      // an unsorted list of this length is sorted first: worth sorting early, beside a recurrence
// `sorted` (2 n words: keys, then positions) from the ids of a table of table_rows rows
int mmda_embed_sort_ids(const int64_t* ids, int n, const int* lengths, int B, int table_rows, unsigned* sorted, void* stream);
// one function per row rule (common.h).  Add: dW[id] += the sum of the id's rows; table_rows is read for a sorted list only
int mmda_embed_list_add(float* dW, const EmbedList& list, int table_rows, void* stream);
// embed_update = sparse.  SparseAdamArgs from the optimizer's scalars: MMDA_EINVAL for a bad pointer / step
int mmda_sparse_adam_args(SparseAdamArgs* out, float* P, float* M, float* V, int table_rows, float lr, float beta1, float beta2, float eps,
                          float clip, float grad_scale, int step);
int mmda_embed_list_sparse_adam(const SparseAdamArgs& ad, const EmbedList& list, void* stream);
// embed_update = deferred.  Update `seq` (Adam step number `step`) of the deferred table update for the rows of an id list: the C ABI's
// mmda_embed_rows_dense_adam with the two things a training step already has, caught-up rows and a sorted list
int mmda_embed_dense_adam_apply(float* P, float* M, float* V, int32_t* row_step, float* step_scalars, int window, const int64_t* ids,
                                const unsigned* sorted, int n, int D, const float* rows, const int32_t* lengths, int B, int table_rows,
                                float lr, float beta1, float beta2, float eps, float clip, float grad_scale, int seq, int step,
                                bool catch_up, void* stream);

// ---- optim.hip
int mmda_zero2(float* a, int64_t na, float* b, int64_t nb, void* stream);      // two buffers cleared by one launch
// The launch behind mmda_clamp_adam, _sum, _runs and _sum_runs: clamp + Adam step h.step over n floats (table == nullptr) or over the
// trainable runs of a table (n unused), with the gradient g or, acc != nullptr, acc + g.  w.flag != nullptr: the launch does not
// complete before *w.flag reaches w.value (flag joins, common.h) and goes out even where there is nothing to update.
// weight_decay > 0: L2 (decoupled == 0) or decoupled decay; scale_dev != nullptr: grad_scale is multiplied by that device float.  The
// three default to "none", where the launch is the one it has always been.
struct AdamHyper { float lr, beta1, beta2, eps, clip, grad_scale; int step; float weight_decay = 0.f; int decoupled = 0; const float* scale_dev = nullptr; };
struct RunTable { const mmda_run* runs; int n_runs; int64_t items; };
struct FlagWait { const unsigned* flag; unsigned value; unsigned* err; };
constexpr FlagWait kNoWait{nullptr, 0u, nullptr};
int mmda_adam_launch(float* p, const float* acc, const float* g, float* m, float* v, int64_t n, const RunTable* table, const AdamHyper& h,
                     const FlagWait& w, void* stream);
// The embedding table walked by stamp.  stamp[r] == epoch: row r is one the step's batch indexes -- the launch that
// reads the step's ids writes the epoch there (RowStamp, below), nothing clears the stamps between steps.  Fewer than 2^31 floats.
struct TableRows { const unsigned* stamp; unsigned epoch; int rows, dim; };
bool mmda_table_rows_ok(const TableRows& t);
// The step's closing launch: mmda_adam_launch's dense stream over the n floats at p / g / m / v, then the rows of the table that FOLLOWS
// them (at float n) whose stamp equals the epoch, gradient read from g.  w: as above.
int mmda_adam_tail_launch(float* p, const float* g, float* m, float* v, int64_t n, const TableRows& t, const AdamHyper& h, const FlagWait& w,
                          void* stream);
// The background pass: step h.step with a zero gradient for the rows of the table at p / m / v whose stamp differs from the epoch, by
// `workgroups` (1 .. 4096) workgroups with non-temporal accesses, each holding lds_bytes of LDS it does not use (0 .. 64 KB: keeps
// them off the CUs of a resident recurrence).  No gradient buffer is read; h.scale_dev must be nullptr.
int mmda_adam_background_launch(float* p, float* m, float* v, const TableRows& t, const AdamHyper& h, int workgroups, int lds_bytes,
                                void* stream);
// What the launch that reads a step's n ids is handed to stamp their rows: stamp[ids[i]] = epoch for every id inside the table
struct RowStamp { unsigned* stamp; unsigned epoch; int table_rows; const int64_t* ids; int n; };
bool mmda_adam_opts_valid(const mmda_adam_opts* o);           // the ranges mmda_misa_set_adam and the *_opts entries accept
// The launches behind mmda_grad_norm: the norm of g (acc + g) over n floats or over a table's runs, block partials in `partials`
// (doubles; mmda_grad_norm_partials sizes it), then norm and clip coefficient in out2[0], out2[1].  An empty range writes 0 and 1.
int mmda_grad_norm_launch(const float* g, const float* acc, int64_t n, const RunTable* table, float max_norm, float grad_scale,
                          double* partials, int64_t partials_capacity, float* out2, void* stream);
// frozen parameters: mmda_runs_build that merges no two ranges across one of `cuts`
int64_t mmda_runs_build_cut(const int64_t* begin, const int64_t* len, int n, int64_t bucket_floats, const int64_t* cuts, int n_cuts,
                            mmda_run* out, int* n_out);
// Adam's bias corrections 1 - beta^t, and from them the two scalars every dense launch of step t is given: lr / (1 - b1^t) and
// 1 / sqrt(1 - b2^t), in double, rounded once
struct BiasCorrections { double bc1, bc2; };
BiasCorrections bias_corrections(float beta1, float beta2, int step);
struct AdamStepScalars { float step_size, inv_bc2_sqrt; };
AdamStepScalars adam_step_scalars(float lr, float beta1, float beta2, int step);

// ---- losses.hip
// mmda_loss_cmd_pairs whose launch, as the last thing it does, sets *flag = value (flag joins, common.h: flag_wait).  Only the
// single-workgroup form can: mmda_loss_cmd_sets_flag says whether a call of that shape will, and a flag given to any other shape is
// MMDA_EINVAL.  flag == nullptr: the plain call.
bool mmda_loss_cmd_sets_flag(int B, int D);
int mmda_loss_cmd_pairs_tail(const float* x, int64_t stride, int nt, int np, const int* pairs_host, int n_moments, int B, int D, float scale,
                             float value_scale, float* loss, float* dx, void* stream, unsigned* flag, unsigned value);

// what mmda_loss_cls_opts, mmda_loss_misc_opts and mmda_misa_set_cls_loss accept for a model of ncls classes (o == nullptr: plain, valid)
bool mmda_cls_opts_valid(const mmda_cls_opts* o, int ncls);
// mmda_loss_misc_opts with the criterion of the handle's task: reg = REG_NONE (loss_terms.h) is that call; else the cls role is the
// regression criterion's, and opts and with_conf must be off
int mmda_loss_misc_reg(const float* scores, const float* tcp, const float* emo, int B, int ncls, float* d_scores, float* d_tcp,
                       int with_conf, int conf_grads, float conf_scale, const float* recon, const float* orig, int64_t n_recon,
                       float recon_scale, float* d_recon, float* d_orig, float* L, float diff_w, float sim_w, float recon_w,
                       float conf_w, int use_conf, const mmda_cls_opts* opts, int reg, void* stream);

// ---- lstm.hip / embed_rows.hip: the launch that reads a step's ids, stamping their rows on its way (st == nullptr: the C ABI's call)
int mmda_lstm_pack_convert_transpose_stamped(int n, const int* H, const float* const* whh, void* const* packed_fwd, void* const* packed_bwd,
                                             void* const* packed_c, const mmda_convert_job* jobs, int njobs, const mmda_transpose_job* tjobs,
                                             int ntjobs, const RowStamp* st, void* stream);
int mmda_embed_gather_stamped(const float* W, const int64_t* ids, int rows, int dim, float* out, const RowStamp* st, void* stream);

// ---- lstm_resident.hip: the resident recurrences of lstm.hip's entry points
int mmda_lstm_cluster_launch(int n, const mmda_lstm_desc* descs, int B, int T, const int32_t* lengths, void* stream, bool bwd,
                             int* used);
