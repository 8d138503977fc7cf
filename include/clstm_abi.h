/*
 * clstm_abi.h -- C ABI of libclstm_hip.so: the MI355X (gfx950) backing of clstm's hot path.
 *
 * This is the drop-in boundary for tmbdev/clstm's per-timestep LSTM forward/backward compute
 * and CTC alignment.  Everything is `extern "C"`, plain pointers and sizes; no C++ or torch
 * types.  All `float*` arguments are DEVICE pointers (hipMalloc / torch.cuda memory) unless the
 * parameter name ends in `_h` (HOST pointer).  All matrices are column-major exactly as the
 * reference's Tensor2 (tensor.h:252,288): element (i, b) of a (rows x cols) batch is
 * ptr[i + rows*b]; a Params matrix W is (no x (1+ni)) with the bias in column 0
 * (tensor.h:263-264).  Functions return 0 on success, non-zero on error;
 * clstm_last_error() returns the message (the reference throws `const char*`, SConstruct:43).
 * Kernels are enqueued on the stream set with clstm_set_stream() (default: the null stream);
 * calls are asynchronous unless stated otherwise.  Handles are not thread-safe (the reference
 * is single-threaded and not re-entrant, batches.cc:11, clstm_compute.cc:47).
 *
 * Two granularities, as SURVEY.md §8(b) requires:
 *  (1) per-op entry points, 1:1 with the DEFGENERIC operator list of clstm_compute.h:72-103
 *      that lies on the 1-D BiLSTM+CTC path (what `clstm_compute.cc` would call per timestep);
 *  (2) fused sequence-level entry points (`clstm_net_*`): what the INetwork layers
 *      (clstm.cc NPLSTM/Parallel/Reversed/Stacked/SoftmaxLayer), ctc.cc and sgd_update actually
 *      use for a whole minibatch of text lines.
 */
#ifndef CLSTM_ABI_H_
#define CLSTM_ABI_H_

#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* nonlinearity codes: clstm_compute.h:10-14 */
enum { CLSTM_LIN = 0, CLSTM_SIG = 1, CLSTM_TANH = 2, CLSTM_RELU = 3, CLSTM_LOGMAG = 4 };

const char* clstm_last_error(void);
int clstm_abi_version(void);
/* stream for every subsequent call on this host thread (a hipStream_t passed as void*) */
int clstm_set_stream(void* hip_stream);
int clstm_synchronize(void);

/* ------------------------------------------------------------------------------------------
 * (1) per-op entry points.  `n`/`m` are the Params dims (rows, cols incl. bias column),
 *     `bs` the batch columns, `len` = rows*bs element counts.
 * ---------------------------------------------------------------------------------------- */
/* forward_nonlin0 / backward_nonlin0   clstm_compute.cc:209-229 / :247-267 */
int clstm_forward_nonlin0(float* y_v, int len, int nl);
int clstm_backward_nonlin0(const float* y_v, float* y_d, int len, int nl);
/* forward_nonlin / backward_nonlin     clstm_compute.cc:130-150 / :168-188 */
int clstm_forward_nonlin(float* y_v, const float* x_v, int len, int nl);
int clstm_backward_nonlin(const float* y_v, const float* y_d, float* x_d, int len, int nl);
/* forward_lin1 / backward_lin1         clstm_compute.cc:275-293 / :294-304 */
int clstm_forward_lin1(float* y_v, const float* W_v, const float* x_v, int n, int m, int bs);
int clstm_backward_lin1(const float* y_d, const float* W_v, float* W_d, const float* x_v, float* x_d,
                        int n, int m, int bs);
/* forward_full1 / backward_full1       clstm_compute.cc:308-314 / :316-320 */
int clstm_forward_full1(float* y_v, const float* W_v, const float* x_v, int n, int m, int bs, int nl);
int clstm_backward_full1(const float* y_v, float* y_d, const float* W_v, float* W_d, const float* x_v,
                         float* x_d, int n, int m, int bs, int nl);
/* forward_softmax / backward_softmax   clstm_compute.cc:324-345 / :346-356 */
int clstm_forward_softmax(float* z_v, const float* W_v, const float* x_v, int n, int m, int bs);
int clstm_backward_softmax(const float* z_d, const float* W_v, float* W_d, const float* x_v,
                           float* x_d, int n, int m, int bs);
/* forward_stack / backward_stack       clstm_compute.cc:360-367 / :368-373 */
int clstm_forward_stack(float* z_v, const float* x_v, const float* y_v, int nx, int ny, int bs);
int clstm_backward_stack(const float* z_d, float* x_d, float* y_d, int nx, int ny, int bs);
/* forward_stack_delay / backward_stack_delay  clstm_compute.cc:377-397 / :398-410
 * ylast_* = y[last].v / y[last].d, or NULL when last < 0 */
int clstm_forward_stack_delay(float* z_v, const float* x_v, const float* ylast_v, int nx, int ny, int bs);
int clstm_backward_stack_delay(const float* z_d, float* x_d, float* ylast_d, int nx, int ny, int bs);
/* forward_reverse / backward_reverse   clstm_compute.cc:414-417 / :418-421
 * on raw Sequence blocks (batches.h:79-86): dims (rows, bs, 2, N); forward copies v AND d */
int clstm_forward_reverse(float* y_seq, const float* x_seq, int rows, int bs, int N);
int clstm_backward_reverse(const float* y_seq, float* x_seq, int rows, int bs, int N);
/* forward_btswitch / backward_btswitch clstm_compute.cc:425-436 / :437-447 (2-D LSTM plumbing, off the 1-D OCR path):
 * x_seq dims (rows, bs, 2, N) -> y_seq dims (rows, N, 2, bs); forward moves .v, backward accumulates .d into x */
int clstm_forward_btswitch(float* y_seq, const float* x_seq, int rows, int bs, int N);
int clstm_backward_btswitch(const float* y_seq, float* x_seq, int rows, int bs, int N);
/* forward_batchstack / backward_batchstack clstm_compute.cc:451-475 / :476-500: x_seq dims (d, bs, 2, N),
 * y_seq dims ((pre+post+1)*d, bs, 2, N); row block pre+k of batch column b holds x's column b+k (zero outside) */
int clstm_forward_batchstack(float* y_seq, const float* x_seq, int d, int bs, int N, int pre, int post);
int clstm_backward_batchstack(const float* y_seq, float* x_seq, int d, int bs, int N, int pre, int post);
/* forward_statemem / backward_statemem clstm_compute.cc:504-508 / :509-515 (last_* NULL if last<0) */
int clstm_forward_statemem(float* state_v, const float* ci_v, const float* gi_v, const float* last_v,
                           const float* gf_v, int len);
int clstm_backward_statemem(const float* state_d, const float* ci_v, float* ci_d, const float* gi_v,
                            float* gi_d, const float* last_v, float* last_d, const float* gf_v,
                            float* gf_d, int len);
/* forward_nonlingate / backward_nonlingate  clstm_compute.cc:530-537 / :539-547 (no heap temp) */
int clstm_forward_nonlingate(float* out_v, const float* state_v, const float* go_v, int len, int nl);
int clstm_backward_nonlingate(const float* out_d, const float* state_v, float* state_d,
                              const float* go_v, float* go_d, int len, int nl);
/* clip_gradient / sgd_update           clstm_compute.cc:553-558 / :560-563 */
int clstm_clip_gradient(float* d, int len, float clip);
int clstm_sgd_update(float* v, float* d, int len, float lr, float mom);

/* ------------------------------------------------------------------------------------------
 * CTC on packed line batches.  A "line batch" is bs text lines packed frame-major:
 * line b owns frames [line_off[b], line_off[b+1]) of a [N][nc] array (nc contiguous).
 * ---------------------------------------------------------------------------------------- */
/* ctc_align_targets(Sequence&, Sequence&, Classes&)  ctc.cc:136-146 (and :57-134), batched.
 * probs/deltas/aligned: DEVICE [N][nc]; aligned may be NULL.  deltas = aligned - probs
 * (clstmhl.h:211-212).  line_off_h[bs+1], states_h (one class per target state, packed),
 * state_off_h[bs+1]: HOST.  Synchronous with respect to the host arrays (they are copied). */
int clstm_ctc_align_batch(const float* probs, float* deltas, float* aligned, int nc,
                          const int* line_off_h, const int* states_h, const int* state_off_h, int bs);
/* Score and force-align candidate transcripts: forward_algorithm (ctc.cc:24-40) over the match scores of ctc_align_targets
 * (ctc.cc:66-77), per (line, candidate) item -- clstm_amd/csrc/ctc_score.h.  probs DEVICE [N][nc]; candidate c has the states
 * [state_off_h[c], state_off_h[c+1]) (one class each, at least one) and belongs to line cand_line_h[c] (NULL: ncand == bs,
 * candidate c <-> line c).  Results, HOST, each may be NULL (at least one must not be):
 *   score_h  [ncand]  lr(T-1, S-1) of the recursion with skip = -5 and the reference's log_add (cut-off at 10).  This is the
 *                     reference's UNNORMALISED score, not the textbook CTC likelihood: every state and frame carries a skip term
 *                     and frame 0 of state 0 counts `same` and `next` both, so a good fit can score slightly above 0.
 *   vscore_h [ncand]  the same recursion with max(same, next) in place of log_add: the score of a best path
 *   path_h   packed   candidate c owns T(line of c) ints, in candidate order: the state occupied at each frame on a best path
 *                     (back-trace from (T-1, S-1): advance iff next > same, ties stay); nondecreasing in steps of 0 or 1, ends in
 *                     S-1; a path that enters state 0 late, at frame i0 > 0, carries -1 on the frames before i0.
 * A line without frames: score = vscore = -INFINITY, no path entries.  A non-finite posterior: non-finite scores for that line's
 * candidates, path entries still in [-1, S).  Everything is validated before anything is enqueued.  Blocking. */
int clstm_ctc_score_batch(const float* probs, int nc, const int* line_off_h, int bs, const int* states_h,
                          const int* state_off_h, const int* cand_line_h, int ncand,
                          float* score_h, float* vscore_h, int* path_h);
/* The n best labellings of every line by CTC prefix beam search in the log domain on the plain posteriors (class 0 = blank,
 * lp = log(max(p, 1e-30f)), f32) -- clstm_amd/csrc/ctc_beam.h states the algorithm.  1 <= nbest <= beam <= 32, nc >= 2, any T.
 * A score is the log-probability the beam gathered for the labelling (a sum over a subset of its paths, so <= its CTC
 * log-likelihood): a true log-probability, NOT comparable with clstm_ctc_score_batch's unnormalised score.
 *   nhyp_h  [bs]         min(nbest, entries alive after the last frame); 0 for a line without frames
 *   score_h [bs*nbest]   hypothesis (b, k) in slot b*nbest + k, best first; unused slots -INFINITY
 *   len_h   [bs*nbest]   labels per hypothesis (<= T_b), unused slots 0; may be NULL
 *   labels_h[nbest*N]    the labels of (b, k): len ints from nbest*line_off[b] + k*T_b, each in [1, nc); may be NULL
 * Ties between candidates are broken by a fixed total order: a line's result does not depend on bs or on the other lines.  A
 * non-finite posterior can make that line's scores non-finite; lengths and labels stay in range, other lines are unaffected. */
int clstm_ctc_beam_batch(const float* probs /*DEVICE [N][nc]*/, int nc, const int* line_off_h, int bs, int beam, int nbest,
                         int* nhyp_h, int* len_h, float* score_h, int* labels_h);
/* A character n-gram language model for the beam search: a dense table lm[ctx][c], HOST float32, nc^(order-1) rows of nc columns.
 * Labels are 1 .. nc-1, 0 = "no label yet".  order 2: ctx = the last label (0 for the empty prefix); order 3: ctx = nc * (the
 * label before last, or 0) + the last label.  Column 0 (blank) is never read.  end_h[nc^(order-1)] (or NULL) is added, weighted,
 * when the hypotheses are ranked after the last frame.  Entries need not be normalised.  Refused: order outside {2, 3}, nc < 2, a
 * table above 2^26 floats, a non-finite entry.  The tables are copied to the device here; the handle belongs to the creating
 * thread's device. */
typedef struct clstm_charlm clstm_charlm;
int clstm_charlm_create(clstm_charlm** out, int order, int nc, const float* table_h, const float* end_h);
int clstm_charlm_destroy(clstm_charlm* lm);
/* clstm_ctc_beam_batch with the language model inside the extension step (clstm_amd/csrc/ctc_beam.h, second part): a prefix's LM
 * value is lm(()) = 0, lm(l + c) = lm(l) + (weight * lm[ctx(l)][c] + bonus) in f32; candidates are selected by
 * logadd(lb', lnb') + lm(prefix), and after the last frame the entries are ranked by tot + lm(l) (+ weight * end[ctx(l)]).  Every
 * class is a candidate of every entry, so the result is that of the algorithm without any class cut.
 *   score_h    [bs*nbest]  the total that was ranked;  am_score_h [bs*nbest] (may be NULL) the acoustic tot, the quantity
 *                          clstm_ctc_beam_batch reports;  nhyp_h, len_h, labels_h as there.
 * Refused before anything is enqueued: lm made for another nc, weight negative or non-finite, bonus non-finite, and
 * beam * (nc - 1) > 4096.  weight = 0, bonus = 0 and no end table give clstm_ctc_beam_batch's bytes. */
int clstm_ctc_beam_lm_batch(const float* probs /*DEVICE [N][nc]*/, int nc, const int* line_off_h, int bs, int beam, int nbest,
                            const clstm_charlm* lm, float weight, float bonus,
                            int* nhyp_h, int* len_h, float* score_h, float* am_score_h, int* labels_h);
/* A lexicon for the beam search (clstm_amd/csrc/ctc_beam.h, third part).  word_class_h[nc] (HOST) flags the classes words are made of;
 * class 0 (blank) is never one, the classes 1 .. nc-1 without the flag are separators.  The nwords words are packed label sequences,
 * word w owns words_h[word_off_h[w] .. word_off_h[w+1]).  A labelling is admissible when every maximal run of word classes in it is a
 * word.  The host builds a trie -- duplicates merged, the children of a node sorted by label, node numbers in the order of the sorted
 * words -- and uploads it once.  Refused, each by name, before anything is uploaded: word_class_h[0] != 0, a label of a word outside
 * 1 .. nc-1 or not a word class, an empty word, decreasing offsets, more than 2^24 labels in all words (a bound on the trie nodes), a
 * device form above 2^28 bytes (4 + nodes * ceil(nc / 32) + nodes + 1 + 2 * edges words).  nwords == 0 is legal: only separators
 * can be written.  The handle belongs to the creating thread's device.
 *   clstm_lexicon_info    info[0..3] = distinct words, trie nodes (the root included), edges, device bytes
 *   clstm_lexicon_admits  HOST only, walks the arrays that were uploaded: *out = 0 labels_h[0..L) is no admissible prefix (or holds a
 *                         label outside 1 .. nc-1), 1 an admissible prefix whose last run is unfinished, 2 an admissible labelling */
typedef struct clstm_lexicon clstm_lexicon;
int clstm_lexicon_create(clstm_lexicon** out, int nc, const unsigned char* word_class_h, const int* words_h, const int* word_off_h,
                         int nwords);
int clstm_lexicon_destroy(clstm_lexicon* lex);
int clstm_lexicon_info(const clstm_lexicon* lex, long long info[4]);
int clstm_lexicon_admits(const clstm_lexicon* lex, const int* labels_h, int L, int* out);
/* clstm_ctc_beam_lm_batch constrained to a lexicon: the same search, expression for expression, except that an extension the lexicon
 * does not allow in the prefix's state is no candidate, and that after the last frame only the entries whose last run is finished are
 * ranked.  lm may be NULL: then the table term is that of an all-zero table (lm(l + c) = lm(l) + bonus) and there is no end table.
 * nhyp_h[b] = min(nbest, admissible live entries) can be 0 for a line WITH frames: then its slots read as a line without frames
 * (len 0, both scores -INFINITY, labels 0).  A lexicon without word classes admits everything: clstm_ctc_beam_lm_batch's bytes (with
 * lm == NULL and bonus == 0, clstm_ctc_beam_batch's).  Refused before anything is enqueued or written: lexicon or model made for
 * another nc, beam * (nc - 1) > 4096, weight negative or non-finite, bonus non-finite, and clstm_ctc_beam_batch's offset / beam /
 * nbest checks. */
int clstm_ctc_beam_lex_batch(const float* probs /*DEVICE [N][nc]*/, int nc, const int* line_off_h, int bs, int beam, int nbest,
                             const clstm_lexicon* lex, const clstm_charlm* lm /*NULL ok*/, float weight, float bonus,
                             int* nhyp_h, int* len_h, float* score_h, float* am_score_h, int* labels_h);
/* Unit-cost Levenshtein distance, the canonical edit script and the confusions of npairs (hypothesis, reference) pairs in one launch
 * (clstm_amd/csrc/edit_distance.h states the algorithm).  Hypotheses: packed ints, pair p owns [hyp_off_h[p], hyp_off_h[p+1]).  References:
 * nref of them, packed, reference q owns [ref_off_h[q], ref_off_h[q+1]).  Pair p is compared with reference ref_of_h[p] (NULL: nref ==
 * npairs, pair p <-> reference p).  Labels lie in [1, nsym); 0 means "nothing" and is refused.  Any lengths, 0 included.  All inputs HOST
 * (copied).  The distance is the reference's levenshtein (clstm.h:329-351).  The script is the canonical one: with D the usual table, from
 * (la, lb), at (i, j): diagonal if i, j > 0 and D[i-1][j-1] + (h[i-1] != r[j-1]) == D[i][j]; else up (i - 1) if i > 0 and D[i-1][j] + 1 ==
 * D[i][j]; else left (j - 1); reported in forward order as codes 0 match, 1 substitution, 2 insertion (a hypothesis symbol with nothing
 * in the reference), 3 deletion (a reference symbol that was not output).  Outputs HOST, each may be NULL, at least one not:
 *   dist_h      [npairs]      the distance
 *   counts_h    [npairs*3]    substitutions, insertions, deletions of the script: their sum is the distance
 *   nops_h      [npairs]      codes in the script (max(la, lb) <= nops <= la + lb)
 *   ops_h                     pair p owns la + lb slots from (hyp_off_h[p] - hyp_off_h[0]) + (sum of lb over the pairs before p); its
 *                             first nops_h[p] slots receive the codes, the others are left as they were
 *   confusion_h [nsym*nsym]   summed over all pairs: [r*nsym + h] per match / substitution, [r*nsym + 0] per deletion, [0*nsym + h] per
 *                             insertion; [0] stays 0
 * dist_h alone keeps no directions.  A pair's results depend on nothing but the pair.  Refused, each by a message that names this entry
 * and the offending index, before anything is enqueued or written: a negative or decreasing offset, a label <= 0 or >= nsym, a ref_of_h
 * entry outside [0, nref), ref_of_h NULL with nref != npairs, nsym < 2, a confusion table above 2^26 ints, every output NULL.  npairs = 0
 * launches nothing (confusion_h is zeroed).  Blocking. */
int clstm_edit_distance_batch(const int* hyp_h, const int* hyp_off_h, int npairs, const int* ref_h, const int* ref_off_h, int nref,
                              const int* ref_of_h, int nsym, int* dist_h, int* counts_h, int* nops_h, int* ops_h, int* confusion_h);
/* mktargets  ctc.cc:148-157: 2L+1 state classes, blank (0) on even positions.  HOST arrays. */
int clstm_mktargets(int* states_h, const int* transcript_h, int L);
/* trivial_decode  ctc.cc:159-190 (+ argmax tensor.h:357-366), batched.  probs DEVICE [N][nc];
 * classes_h/locs_h HOST [N] (line b's result starts at line_off[b]); counts_h HOST [bs].
 * Blocking. */
int clstm_trivial_decode_batch(const float* probs, int nc, const int* line_off_h, int bs,
                               int* classes_h, int* locs_h, int* counts_h);

/* ------------------------------------------------------------------------------------------
 * (2) fused network: Stacked{ Parallel{NPLSTM, Reversed{NPLSTM}} x nlayers, SoftmaxLayer }
 *     = prefab "bidi" / "bidi2" (clstm_prefab.cc:52-68, 86-109); unidirectional = "lstm1".
 * ---------------------------------------------------------------------------------------- */
typedef struct clstm_net clstm_net;
#define CLSTM_MAX_LAYERS 4
typedef struct {
  int nlayers;                    /* BiLSTM layers (1 = bidi, 2 = bidi2) */
  int unidirectional;             /* 1: Stacked{NPLSTM, Softmax} (lstm1) */
  int ninput;                     /* features per frame (48 for OCR lines) */
  int nhidden[CLSTM_MAX_LAYERS];  /* NPLSTM units per direction */
  int nclasses;                   /* softmax outputs */
} clstm_net_desc;

/* Number of floats of the flat parameter buffer: exactly n_params() (clstm.cc:852-857) in
 * walk_params order (clstm.cc:59-62): per NPLSTM WCI,WGF,WGI,WGO (std::map order), forward
 * before reversed, layers in order, softmax W1 last; each Params block column-major. */
int clstm_net_nparams_for(const clstm_net_desc* desc);
/* params_d / derivs_d / grads_d: caller-owned DEVICE buffers of nparams floats (the analogue of
 * share_params, clstm.cc:859-870), or NULL to let the library allocate.
 *   params = Params.v ; derivs = Params.d (gradient + carried momentum, clstm_compute.cc:560-563);
 *   grads  = this step's fresh minibatch gradient sum (what data-parallel ranks all-reduce). */
int clstm_net_create(clstm_net** out, const clstm_net_desc* desc, float* params_d, float* derivs_d,
                     float* grads_d);
int clstm_net_destroy(clstm_net* net);
/* Precision of the hoisted gate GEMMs (W_x.x for all frames, the weight-gradient and input-delta GEMMs):
 *   0 (default) exact f32 MFMA -- the parity path (1e-4 on activations);
 *   1           bf16 inputs, f32 accumulation (v_mfma_f32_16x16x32_bf16) in those GEMMs; the recurrence, softmax
 *               and CTC stay f32;
 *   2           1 + bf16 MFMA operands (recurrent weights, h, gate deltas) inside the lock-step recurrence of
 *               layers wider than 128 cells (csrc/lstm_wide.h: lstm_xcd_*_bf16) -- what BASELINE config "2 x BiLSTM(512),
 *               bf16 MFMA" names; accumulation, cell state, softmax and CTC stay f32.  Not parity modes.
 * Layers wider than 128 cells run their recurrence as ONE persistent launch per pass in every mode (a workgroup group
 * per XCD, csrc/lstm_wide.h; environment CLSTM_XCD_REC=0: one launch per time step); in modes 0 and 1 with f32 operands
 * and results bit-identical to the per-step kernels. */
int clstm_net_set_gemm_precision(clstm_net* net, int mode);
int clstm_net_nparams(clstm_net* net);
int clstm_net_buffers(clstm_net* net, float** params_d, float** derivs_d, float** grads_d);
/* get_params/set_params/get_derivs/set_derivs (clstm.cc:872-917): HOST buffers, blocking. */
int clstm_net_set_params_h(clstm_net* net, const float* params_h);
int clstm_net_get_params_h(clstm_net* net, float* params_h);
int clstm_net_set_derivs_h(clstm_net* net, const float* derivs_h);
int clstm_net_get_derivs_h(clstm_net* net, float* derivs_h);
int clstm_net_get_grads_h(clstm_net* net, float* grads_h);
/* must be called after writing the params buffer directly on the device */
int clstm_net_params_changed(clstm_net* net);
/* INetwork::setLearningRate (clstm.cc:158-161) + gradient_clip attr (clstm.cc:204) */
int clstm_net_set_learning_rate(clstm_net* net, float lr, float momentum);
/* What every update clamps to +-clip is derivs + grads (the carried momentum plus the fresh minibatch gradient), before the momentum
 * multiply, as the reference does (clstm.cc:201-217); a clip >= 1e6 switches the clamp off.  clip must be > 0 (0, a negative value
 * and NaN are refused and the previous clip stays in force). */
int clstm_net_set_gradient_clip(clstm_net* net, float clip);

/* What the per-minibatch entry points need of the net.  The net keeps one record of the minibatch it holds (clstm_debug_net_holds) and every
 * entry below states its needs against it in one line (csrc/net.inc: Net::require); a need that is not met is refused by its text:
 *   batch declared            else "set_batch first"
 *   current (no declared next) else "no current minibatch: ..." -- between a clstm_net_train_step_next that declared its next minibatch and
 *                             the call that brings, adopts or drops it, the geometry is that NEXT minibatch's and no outputs of it exist
 *   saved (not predict's)     else "<entry>: the current minibatch was computed by clstm_net_predict, which saves nothing for a backward pass ..."
 *   backward ran              else "input deltas not enabled / no backward yet" (clstm_net_enable_input_deltas, then a backward pass of THIS minibatch)
 *
 *   entry                                              | batch declared | current (no declared next) | saved (not predict's) | backward ran
 *   get_outputs_h, decode, score, beam, beam_lm,       |                |                            |                       |
 *   beam_lex, errors                                   | yes           | yes                        |                       |
 *   get_state_h which = 5                              | yes            | yes                        |                       |
 *   get_state_h other, ctc, backward                   | yes            | yes                        | yes                   |
 *   set_output_deltas_h                                | yes            | yes                        | yes                   |
 *   n_states, get_states_h                             | yes            | yes                        | yes                   |
 *   get_input_deltas_h (+ enabled)                     | yes            | yes                        | yes                   | yes
 *   set_inputs_h, set_inputs_d, forward                | yes            | adopt / drop               |                       |
 *
 * adopt / drop: clstm_net_forward and clstm_net_set_inputs_* ADOPT a declared next minibatch -- it becomes the current one (forward computes
 * its outputs from the frames the declaring step ingested; set_inputs_* replaces those frames), and a later step call that brings it declares
 * and ingests it again, with identical results.  clstm_net_set_batch, clstm_net_predict, clstm_net_set_states_h and a step call that brings
 * another minibatch DROP it. */
/* Declare the next minibatch: bs lines of T_h[b] frames each (HOST).  N = sum T.  T_h / bs are validated before the net is touched
 * (no negative length, at least one frame, fewer than 2147483000): a refused call leaves the previous minibatch the current one. */
int clstm_net_set_batch(clstm_net* net, const int* T_h, int bs);
/* set_inputs (clstm.cc:684-690): x [N][ninput], frame-major, feature contiguous.
 * Input range: any float32.  The result class does not depend on the minibatch size: the batched recurrence that single-layer
 * narrow nets take from 640 lines per GPU on (csrc/lstm_mfma.h) scales its operands for |x| <= 255 -- normalised text lines are
 * in [0, 1] -- and a minibatch that holds a larger or a non-finite input is computed by the per-line f32 kernels of smaller
 * minibatches instead, at their speed.  The device decides (no host synchronisation; csrc/lstm_mfma.h "Input range");
 * clstm_debug_path_count(21) counts the minibatches that went that way.  A non-finite pixel stays what it is on every path:
 * non-finite outputs, the update skipped and reported (clstm_last_error). */
int clstm_net_set_inputs_h(clstm_net* net, const float* x_h);
int clstm_net_set_inputs_d(clstm_net* net, const float* x_d);
/* net->forward() */
int clstm_net_forward(clstm_net* net);
/* net->outputs: DEVICE pointer to [N][nclasses] softmax outputs / their deltas (.d plane) */
int clstm_net_outputs(clstm_net* net, float** probs_d, float** deltas_d);
int clstm_net_get_outputs_h(clstm_net* net, float* probs_h);
int clstm_net_set_output_deltas_h(clstm_net* net, const float* deltas_h);
/* CLSTMOCR::fwdbwd CTC leg (clstmhl.h:207-212): mktargets + ctc_align_targets + deltas for
 * every line of the batch.  labels_h packed transcripts, L_h[bs] lengths (HOST).
 * aligned_h (HOST, [N][nc]) may be NULL. */
int clstm_net_ctc(clstm_net* net, const int* labels_h, const int* L_h, float* aligned_h);
/* clstm_ctc_score_batch on the outputs of the net's current minibatch: labels_h packed transcripts, L_h[ncand]; mktargets is
 * applied per candidate; cand_line_h[ncand] names each candidate's line (NULL: one per line, ncand == bs).  Needs a current
 * minibatch; reads the outputs only, so it works after clstm_net_forward, after a training step and after clstm_net_predict.
 * Rank-local with a communicator attached.  Deltas, gradients, parameters, the step count, the device error words and a declared
 * next minibatch are untouched.  Kernel time under "ctc_score" (clstm_net_kernel_time_ms). */
int clstm_net_score(clstm_net* net, const int* labels_h, const int* L_h, const int* cand_line_h, int ncand,
                    float* score_h, float* vscore_h, int* path_h);
/* clstm_ctc_beam_batch on the outputs of the net's current minibatch.  Exactly the preconditions and guarantees of clstm_net_score:
 * needs a current minibatch; works after clstm_net_forward, after a training step and after clstm_net_predict; rank-local;
 * parameters, derivs, grads, deltas, the step count, the device error words and a declared next minibatch are untouched.  Kernel
 * time under "ctc_beam". */
int clstm_net_beam(clstm_net* net, int beam, int nbest, int* nhyp_h, int* len_h, float* score_h, int* labels_h);
/* clstm_ctc_beam_lm_batch on the outputs of the net's current minibatch: the preconditions and guarantees of clstm_net_beam.  Kernel
 * time under "ctc_beam_lm". */
int clstm_net_beam_lm(clstm_net* net, int beam, int nbest, const clstm_charlm* lm, float weight, float bonus,
                      int* nhyp_h, int* len_h, float* score_h, float* am_score_h, int* labels_h);
/* clstm_ctc_beam_lex_batch on the outputs of the net's current minibatch (lm may be NULL): the preconditions and guarantees of
 * clstm_net_beam.  Kernel time under "ctc_beam_lex". */
int clstm_net_beam_lex(clstm_net* net, int beam, int nbest, const clstm_lexicon* lex, const clstm_charlm* lm, float weight, float bonus,
                       int* nhyp_h, int* len_h, float* score_h, float* am_score_h, int* labels_h);
/* clstm_edit_distance_batch for the net's current minibatch: the hypotheses are trivial_decode of every line, compared where
 * decode_kernel leaves them on the device (nothing comes to the host but the results); the references are labels_h / L_h[bs], one packed
 * transcript per line, with nsym = nclasses + 1 -- label nclasses, allowed in references only, stands for a character outside the codec and
 * matches nothing.  dist_h [bs], counts_h [bs*3], confusion_h [(nclasses+1)^2] as there; each may be NULL, at least one not.  Exactly
 * the preconditions and guarantees of clstm_net_score: needs a current minibatch; works after clstm_net_forward, after a training step
 * and after clstm_net_predict; rank-local; parameters, derivs, grads, deltas, the step count, the device error words and a declared next
 * minibatch are untouched.  Refusals as clstm_edit_distance_batch's, by this entry's name.  Kernel time under "edit_distance". */
int clstm_net_errors(clstm_net* net, const int* labels_h, const int* L_h, int* dist_h, int* counts_h, int* confusion_h);
/* net->backward(): accumulates this minibatch's gradient sum into grads (zeroed first). */
int clstm_net_backward(clstm_net* net);
/* input deltas of the first layer are only computed if enabled (nothing on the OCR path reads
 * them; the gradient tests do). */
int clstm_net_enable_input_deltas(clstm_net* net, int on);
int clstm_net_get_input_deltas_h(clstm_net* net, float* dx_h);
/* sgd_update(Network) (clstm.cc:201-217) on the flat buffers:
 *   derivs += grads ; derivs = clip(derivs, +-gradient_clip) ; params += lr*derivs ;
 *   derivs *= momentum.   (lr is NOT normalised, see SURVEY.md §7 "lr normalisation".) */
int clstm_net_update(clstm_net* net);
/* trivial_decode of every line; HOST outputs as clstm_trivial_decode_batch.  Blocking. */
int clstm_net_decode(clstm_net* net, int* classes_h, int* locs_h, int* counts_h);
/* CLSTMOCR::predict (clstmhl.h:225-262) for a whole minibatch in ONE call: declare the minibatch (T_h[bs] line lengths, HOST), take
 * its frames (x_d DEVICE / x_h HOST, [sum T][ninput]), run the forward pass and trivial_decode.  Blocking: it returns results.
 *   Outputs (HOST) are laid out as clstm_net_decode's: line b's entries start at its first frame's index, counts_h[b] of them;
 * conf_h[i] is the softmax output at (locs_h[i], classes_h[i]) -- CharPrediction::p.  classes_h / locs_h / conf_h may be NULL,
 * counts_h is required.
 *   The forward pass is the one clstm_net_forward runs for this minibatch -- one scheduler, one rule for the kernel family (fused
 * launch, batched MFMA recurrence from 640 lines on with its input-range routing, per-line kernels; clstm_net_set_strict_f32 and
 * the forced experiment options apply) -- in its NO-SAVE form: identical arithmetic, bit-identical outputs, but nothing is kept for
 * a backward pass (no gate activations, no cell states, no source rows) and the buffers only a training step needs are not even
 * reserved (clstm_net_device_bytes).  Nets with a wide layer (> 128 cells) or in a bf16 mode (clstm_net_set_gemm_precision) have
 * no no-save kernels: predict runs their ordinary forward pass.  T_h / bs are validated before the net is touched.
 *   Afterwards the minibatch is the net's current one: clstm_net_outputs, clstm_net_get_outputs_h, clstm_net_decode and
 * clstm_net_get_state_h(which = 5) work; clstm_net_ctc, clstm_net_backward, clstm_net_set_output_deltas_h, clstm_net_get_state_h
 * (other `which`), clstm_net_n_states / clstm_net_get_states_h and clstm_net_get_input_deltas_h refuse and name clstm_net_predict;
 * clstm_net_forward (and clstm_net_set_inputs_*) reserve what a training pass needs and go on as usual.
 *   Training state is untouched: parameters, derivs, grads, the step count, the device error words (a non-finite pixel gives
 * non-finite outputs and arms nothing, whatever clstm_net_set_training says).  A minibatch declared by clstm_net_train_step_next is
 * dropped exactly as by clstm_net_set_batch: the next step takes the ordinary path with identical results.  With a communicator
 * attached predict is rank-local (no collective). */
int clstm_net_predict(clstm_net* net, const int* T_h, int bs, const float* x_d, int* classes_h, int* locs_h, float* conf_h,
                      int* counts_h);
int clstm_net_predict_h(clstm_net* net, const int* T_h, int bs, const float* x_h, int* classes_h, int* locs_h, float* conf_h,
                        int* counts_h);
/* ------------------------------------------------------------------------------------------
 * Line normalisation on the device: CenterNormalizer::measure + normalize (extras.cc:53-131, 205-285; restated in
 * clstm_amd/host/normalizer.h) for a minibatch of RAW line images, bit for bit what the host code gives (csrc/normalize.h): the
 * frames are the bytes, T and r the values, of the host normaliser.  Everything is enqueued on the library's one stream.
 *   Images: ink = 1 (1 - pixel of the PNG, clstmocrtrain.cc:73), float32 in the host Image layout -- pixel (x = i, y = j) of a
 * w x h line at i*h + j -- packed back to back; w_h[bs], h_h[bs]: HOST.
 *   Limit: the reach of every Gaussian mask, 1 + int(3 sigma) for sigma = h/2, h*smooth2d and h*smooth1d, must not exceed 800
 * (any h <= 256 at the default parameters smooth2d = 1, smooth1d = 0.3; h <= 532 for smooth2d <= 0.5); a line beyond it is
 * refused by name.  A line may have any width whose buffers fit in device memory (up to 2^30 pixels).
 * ---------------------------------------------------------------------------------------- */
typedef struct clstm_normalizer clstm_normalizer;
/* the reference's defaults: target_height 48, smooth2d 1.0, smooth1d 0.3, range 4.0.  target_height >= 1 */
int clstm_normalizer_create(clstm_normalizer** out, int target_height, float smooth2d, float smooth1d, float range);
int clstm_normalizer_destroy(clstm_normalizer* nz);
/* measure + normalize of bs lines.  pix_h: HOST, packed as above; w_h / h_h[bs] HOST.  T_h[bs] out: frames per line; r_h[bs] out
 * (CenterNormalizer::r), may be NULL.  Blocking only for the bs values of r / T (two floats per line are read back; mad, r and the
 * target width are computed on the host).  *frames_d: library-owned DEVICE [sum T][target_height], line after line -- what
 * clstm_net_set_inputs_d, clstm_net_predict and clstm_net_train_step take -- valid until the next call on this normalizer; the warp
 * kernel is enqueued on the library's stream before the call returns.
 *   bs > 0 and every w, h >= 1 (and the limit above) are checked before anything is touched.  A line without ink (the sum of its
 * pixels is 0: the host's int(NaN) is undefined there) or with a non-finite mean absolute deviation is refused after the measure
 * stage: clstm_last_error names the line index, no frames are produced for the call (T_h / r_h are not written), and the
 * normalizer stays usable. */
int clstm_normalizer_run_h(clstm_normalizer* nz, const float* pix_h, const int* w_h, const int* h_h, int bs, int* T_h, float* r_h,
                           float** frames_d);
/* the same with the pixels already on the device (pix_d DEVICE; not modified) */
int clstm_normalizer_run_d(clstm_normalizer* nz, const float* pix_d, const int* w_h, const int* h_h, int bs, int* T_h, float* r_h,
                           float** frames_d);
/* blocking copy of the last call's frames, HOST [sum T][target_height]; refused if that call produced none */
int clstm_normalizer_get_frames_h(clstm_normalizer* nz, float* frames_h);
/* bytes of the normalizer's grow-only device buffers: the frames (sized after the T read-back; they grow and never shrink), the
 * uploaded pixels, two intermediate images, the per-column arrays, masks and item lists */
int clstm_normalizer_device_bytes(clstm_normalizer* nz, long long* bytes);

/* ------------------------------------------------------------------------------------------
 * Line degradation on the device, for training: a minibatch of RAW line images in, the same number of images of the same sizes
 * out -- a small elastic distortion, an affine jitter, a little blur -- bit for bit what degrade_line of clstm_amd/host/degrade.h
 * (the specification: noise fields from an integer hash, gauss2d, min / max bounding, bilinear warp with background outside,
 * gauss2d) gives.  The output has the packed layout clstm_normalizer_run_d takes (ink = 1, pixel (x = i, y = j) of a line at
 * pix + i*h + j, lines back to back).  Everything is enqueued on the library's one stream.
 *   Per line: m[4], tx, ty -- output pixel (i, j) is read at x = m0 (i - cx) + m1 (j - cy) + cx + tx + d0, y alike from m2, m3, ty,
 * d1, about the centre cx = (w - 1)/2, cy = (h - 1)/2; sigma, maxdelta -- the displacement fields d0, d1 are noise smoothed with sigma
 * and scaled into [-maxdelta, maxdelta] (maxdelta = 0: no distortion, sigma is not used); blur -- the sigma of the final Gaussian
 * (0: none); seed -- of the line's noise.  m = {1, 0, 0, 1}, tx = ty = maxdelta = blur = 0 gives the input back byte for byte.
 *   Limits, refused by name before anything is touched: bs > 0; every w, h >= 1, at most 2^23, w*h <= 2^30; m, tx, ty, sigma finite;
 * maxdelta and blur finite and >= 0; sigma > 0 where maxdelta > 0; 1 + int(3 sigma) <= 800 (NZ_MAXRANGE) for sigma (where used)
 * and blur.  A refused call produces nothing and leaves the degrader usable.
 * ---------------------------------------------------------------------------------------- */
typedef struct clstm_degrader clstm_degrader;
typedef struct { float m[4]; float tx, ty; float sigma, maxdelta; float blur; unsigned seed; } clstm_degrade_line;
/* the ranges clstm_degrade_draw draws within: rotation in +-angle (radians), log of the scale in +-scale, log of the x/y anisotropy
 * in +-aniso, shift in +-translate*h pixels along each axis; sigma, maxdelta (pixels), blur in [LO, HI] */
typedef struct { float angle, scale, aniso, translate; float sigma[2], maxdelta[2], blur[2]; } clstm_degrade_ranges;
int clstm_degrader_create(clstm_degrader** out);
int clstm_degrader_destroy(clstm_degrader* dg);
/* pix_h: HOST, packed as above; w_h / h_h[bs], lines_h[bs]: HOST.  *out_pix_d: library-owned DEVICE, the degraded lines packed like
 * the input -- what clstm_normalizer_run_d takes -- valid until the next call on this degrader.  Asynchronous. */
int clstm_degrader_run_h(clstm_degrader* dg, const float* pix_h, const int* w_h, const int* h_h, int bs, const clstm_degrade_line* lines_h,
                         float** out_pix_d);
/* the same with the pixels already on the device (pix_d DEVICE; not modified).  No host synchronisation: the per-call arrays go up
 * in one copy from pinned memory, the minimum and maximum of the noise fields stay on the device.  (A buffer that has to grow
 * drains the stream once; buffers never shrink.) */
int clstm_degrader_run_d(clstm_degrader* dg, const float* pix_d, const int* w_h, const int* h_h, int bs, const clstm_degrade_line* lines_h,
                         float** out_pix_d);
/* blocking copy of the last call's output, HOST [sum w*h]; refused if that call produced nothing */
int clstm_degrader_get_pixels_h(clstm_degrader* dg, float* out_h);
/* bytes of the degrader's grow-only device buffers: the output, the two noise fields of every distorted line after each filter pass,
 * the blur's intermediate image, the uploaded pixels of run_h, the min / max partials, the per-call block */
int clstm_degrader_device_bytes(clstm_degrader* dg, long long* bytes);
/* Host only.  The default ranges, mild enough that a line stays legible: angle 0.02 rad (1.1 degrees), scale 0.03, aniso 0.02,
 * translate 0.03 (of the height), sigma [3, 8], maxdelta [0, 1.5] pixels, blur [0, 0.7]. */
int clstm_degrade_default_ranges(clstm_degrade_ranges* out);
/* Host only.  THE statement of how a line's parameters are drawn: a counter-based generator (splitmix64's finaliser chained over seed,
 * key, visit; csrc/degrade_run.inc) draws, uniformly within rg, the angle, the log-scale ls, the anisotropy an, tx, ty, sigma, maxdelta,
 * blur and the noise seed; m = {c sx, -s sy, s sx, c sy} with sx = exp(ls + an), sy = exp(ls - an), c, s = cos, sin of the angle, in
 * double, rounded to float once -- the device never evaluates a transcendental.  key is the caller's name for the line (its index in
 * the training set), NOT its position in the minibatch; visit counts how often it has been drawn: what a line becomes does not depend
 * on which lines it is batched with.  Ranges of zero width give the identity parameters exactly. */
int clstm_degrade_draw(unsigned long long seed, unsigned long long key, unsigned long long visit, const clstm_degrade_ranges* rg, int w, int h,
                       clstm_degrade_line* out);

/* sum of the net's device allocations in bytes (parameters, packed weights, every per-minibatch buffer, CTC / decode scratch) */
int clstm_net_device_bytes(clstm_net* net, long long* bytes);
/* internal NPLSTM state for parity tests: which = 0 gi,1 gf,2 go,3 ci,4 state,5 output h,
 * 6 gate delta gi,7 gf,8 go,9 ci (pre-activation deltas after backward_nonlin0).
 * dir 0 = forward NPLSTM, 1 = the NPLSTM inside Reversed.  out_h: HOST [N][nhidden] in FRAME
 * order (i.e. already un-reversed).  Blocking. */
int clstm_net_get_state_h(clstm_net* net, int layer, int dir, int which, float* out_h);
/* name and device time (ms) of the forward/backward kernels since the last reset -- used by bench.py for the roofline
 * object.  Enable with clstm_net_enable_timing(net, 1).  While it is on, every launch carries a start / stop event pair
 * bound to its own dispatch packet (hipExtLaunchKernel): the time is the kernel's duration by the packet's own time
 * stamps, the figure rocprofv3 --kernel-trace reports; nothing is inserted into the stream.  total_ms sums the launches
 * of every phase of that name, launches counts the phases. */
/* The weight-gradient GEMM of a narrow BiLSTM layer runs beside the backward recurrence (csrc/gemm_dw.h):
 * mode 0: off (GEMM after the recurrence); 1 (default): both as two workgroup roles of ONE launch
 * (csrc/lstm_bwd_dw.h) for batches large enough to profit; 2: the same always (tests); 3: two launches on streams
 * with complementary CU masks (measured slower than mode 0, kept for the record).  Results are the same sums in a
 * different slab order; in modes 1-3 the products run on the bf16 MFMA with both f32 operands split EXACTLY into three
 * bf16 terms (x1 + x2 + x3 = x; the six products of weight >= 2^-16 summed in f32: what is dropped is < 2^-23 |x||y| per
 * product, the size of an f32 multiply's own rounding; experiment options CLSTM_DEBUG="split_terms=2" -- two terms, three
 * products, < 2^-16 -- and "dw_x3=0" -- the f32 MFMA), and the top layer's launch also computes the softmax layer's W.d.  stats: overlapped backward passes so far; slabs that gave up waiting for the recurrence
 * (must stay 0). */
int clstm_net_set_overlap(clstm_net* net, int mode);
int clstm_net_get_overlap(clstm_net* net, int* mode);   /* the current mode (default: environment CLSTM_OVERLAP, else 1) */
/* on != 0: every product of the training step on the f32 MFMA -- the backward products that default to operand-exact split
 * products on the bf16 MFMA (weight gradients, the softmax layer's W.d / x.d) included, and no batched split-product recurrence
 * (csrc/lstm_mfma.h f16 x 2, csrc/lstm_mfma_bwd.h bf16 x 2) by the library's own rule at any minibatch size: a strict net of 640
 * lines and more keeps the per-line f32 kernels.  Same as CLSTM_DEBUG="dw_x3=0,gemm_x3=0,fwd_mfma=0,bwd_mfma=0", per net
 * (bench.py's `strict_f32` leg and --strict-f32).  An experiment option that FORCES a kernel family (CLSTM_DEBUG /
 * clstm_debug_set_option "fwd_mfma=2", "bwd_mfma=2": tests) wins over this flag. */
int clstm_net_set_strict_f32(clstm_net* net, int on);
int clstm_net_overlap_stats(clstm_net* net, long long* launches, int* timeouts);
int clstm_net_enable_timing(clstm_net* net, int on);
int clstm_net_kernel_time_ms(clstm_net* net, const char* kernel_name, double* total_ms, int* launches);
int clstm_net_reset_timing(clstm_net* net);

/* CLSTMOCR::train (clstmhl.h:201-223) for a whole minibatch in ONE call: set_batch + set_inputs_d + forward +
 * ctc + backward + [all-reduce of grads when a communicator is attached] + update, enqueued on the library
 * stream without any host synchronisation.  T_h[bs], labels_h (packed transcripts), L_h[bs]: HOST;
 * x_d: DEVICE [sum T][ninput].  Decode with clstm_net_decode() afterwards if the caller wants the output. */
int clstm_net_train_step(clstm_net* net, const int* T_h, int bs, const float* x_d, const int* labels_h,
                         const int* L_h);
/* clstm_net_train_step for a loop that knows its NEXT minibatch (a data loader one minibatch ahead: what clstmocrtrain's
 * sample loop, clstmocrtrain.cc:167-172, is once its lines are batched).  Tn_h / bsn / xn_d / labels_n_h / Ln_h describe the
 * minibatch of the next call in the same form (all NULL / 0: exactly clstm_net_train_step).  The front half of that next step --
 * batch geometry, the host half of its alignment, the copy of its frames into the net's input block, of its line offsets and CTC
 * metadata -- is done by THIS call: by extra workgroups of this step's last launch (slab reduction + update), so the next
 * call starts with its forward launch (one launch less per step: 5.7 us of a 64 x 200 step).  The next call must pass the same
 * x pointer and the same T / transcripts (compared by content) to profit; anything else -- another minibatch after all, a
 * communicator of several ranks, clstm_net_set_batch in between -- silently takes the ordinary path.  xn_d must stay unchanged
 * from this call on.  Until the next step the net has no current minibatch: every entry of the table above clstm_net_set_batch that needs
 * a current one refuses; clstm_net_forward and clstm_net_set_inputs_* adopt the declared minibatch.  A next minibatch that would be
 * refused (a negative line length, no frames, a blank or out-of-range label, an alignment that does not fit) is found on the host before
 * anything is touched: this step completes as clstm_net_train_step, its minibatch stays the current one with its outputs addressable,
 * and the call that brings the bad minibatch reports the error.  Results are bit-identical to clstm_net_train_step's. */
int clstm_net_train_step_next(clstm_net* net, const int* T_h, int bs, const float* x_d, const int* labels_h, const int* L_h,
                              const int* Tn_h, int bsn, const float* xn_d, const int* labels_n_h, const int* Ln_h);
/* The same step fed from HOST memory (what clstmocrtrain has after read_png + CenterNormalizer, clstmocrtrain.cc:167-172,
 * extras.cc:227-285): x_h: [sum T][ninput].  Asynchronous: the frames go to the device on a copy stream (a DMA from
 * x_h itself if it is pinned -- clstm_host_alloc -- else through a pinned staging buffer of the library) into one of two
 * device input buffers, overlapping the previous step's kernels; the call returns once everything is enqueued.  x_h may
 * be reused when the call returns if it is pageable, after the NEXT call returns if it is pinned (two buffers in
 * flight). */
int clstm_net_train_step_h(clstm_net* net, const int* T_h, int bs, const float* x_h, const int* labels_h,
                           const int* L_h);
/* pinned host memory for the above */
int clstm_host_alloc(void** p, size_t bytes);
int clstm_host_free(void* p);

/* State externalisation: n_states / get_states / set_states (clstm.cc:762-811; upstream test
 * test-lstm2.cc:79-142).  The reference walks every `Sequence` state of every layer (walk_states,
 * clstm.cc:64-67: per NPLSTM the std::map order ci, gf, gi, go, source, state, then the layer's
 * inputs/outputs are NOT states) and copies the .v planes.  Here: the same order and contents for the
 * current minibatch, per layer: forward NPLSTM then the NPLSTM inside Reversed (in ITS time order, i.e.
 * frame T-1-t at its step t), each state as [T][rows][bs] flattened exactly as Sequence::v would be for a
 * bs=1 line batch; for bs>1 lines are concatenated line after line.  `source` = [x_t ; h_{t-1}] rows
 * (clstm_compute.cc:377-397).  HOST buffers, blocking. */
int clstm_net_n_states(clstm_net* net, long long* n);
int clstm_net_get_states_h(clstm_net* net, float* states_h, long long n);
int clstm_net_set_states_h(clstm_net* net, const float* states_h, long long n);

/* ------------------------------------------------------------------------------------------
 * Data-parallel exchange: every GPU owns an independent shard of the minibatch's lines; the
 * ONE exchange is an all-reduce (sum, fp32) of the flat fresh-gradient buffer before the identical update on
 * every rank.  Reference precedent: share_deltas (clstm.cc:731-744) -- which sums Params.d, momentum
 * included; here only the fresh gradient crosses GPUs (clstm_net_create: grads_d).
 * RCCL (librccl.so.1) is bound at first use; one communicator per process = per GPU (hipSetDevice first).
 * ---------------------------------------------------------------------------------------- */
typedef struct clstm_comm clstm_comm;
#define CLSTM_COMM_ID_BYTES 128
/* rank 0: ncclGetUniqueId into id_h[CLSTM_COMM_ID_BYTES]; ship the bytes to the other ranks by any means */
int clstm_comm_unique_id(char* id_h);
/* collective over all ranks (ncclCommInitRank on the current device) */
int clstm_comm_create(clstm_comm** out, const char* id_h, int rank, int nranks);
int clstm_comm_destroy(clstm_comm* comm);
int clstm_comm_rank(clstm_comm* comm);
int clstm_comm_size(clstm_comm* comm);
/* 1 once the ranks have mapped each other's exchange buffers (HIP IPC; decided collectively at the first clstm_net_train_step with
 * the communicator attached): clstm_net_train_step then runs the peer-read all-reduce fused into the update -- one-shot (every
 * rank sums every rank's whole buffer) for gradients up to 4 MB and at two ranks, two-phase (reduce-scatter, then all-gather
 * inside the update kernel) above 4 MB at three or more ranks; the exchange buffers grow, collectively, to the largest gradient
 * seen.  Environment CLSTM_PEER_ALLREDUCE=0: always ncclAllReduce + update.  0: ncclAllReduce (also after a set-up, the first or a
 * later, larger one, that did not succeed on every rank). */
int clstm_comm_peer_active(clstm_comm* comm);
/* floats: what one exchange buffer of the peer path holds at present (at least 1 << 20 once it is up; it grows when a larger
 * gradient arrives and never shrinks); 0 before the set-up and while clstm_comm_peer_active is 0. */
int clstm_comm_peer_capacity(clstm_comm* comm, long long* floats);
/* in-place sum over ranks of buf_d[0..n) (DEVICE, f32), enqueued on the library stream: no cross-stream
 * event, no host synchronisation. */
int clstm_allreduce_flat(clstm_comm* comm, float* buf_d, long long n);
/* attach (or detach with NULL) a communicator: clstm_net_update() / clstm_net_train_step() then all-reduce
 * the fresh gradient buffer `grads` before derivs += grads. */
int clstm_net_set_comm(clstm_net* net, clstm_comm* comm);
/* Replica consistency (the reference RE-SYNCHRONISES its replicas, distribute_weights / average_weights, clstm.cc:718-729,
 * 746-760; here every rank applies the identical update to the identical all-reduced gradient, so the replicas must stay
 * bit-identical and that is CHECKED): enqueue a parameter checksum, its all-reduce over the attached communicator and the
 * comparison sum == nranks * own.  A mismatch raises a sticky device error (no later update is applied) that the next
 * synchronisation point reports as "replicas diverged ... at training step N".  Called by the library itself every
 * CLSTM_REPLICA_CHECK_EVERY (default 256, 0: never) updates of a net whose communicator has several ranks; collective: every
 * rank must call it at the same point.  No-op without such a communicator. */
int clstm_net_replica_check(clstm_net* net);
/* on = 0: forward passes of this net belong to no training step (CLSTMOCR::predict, the test-set pass of clstmocrtrain,
 * clstmhl.h:225-253): a non-finite logit there does not arm the device NaN / Inf flag that blocks updates (the reference only
 * asserts in backward, clstm.cc:630-649).  Default 1. */
int clstm_net_set_training(clstm_net* net, int on);

/* ------------------------------------------------------------------------------------------
 * diagnostics (used by tests/ to pin the hardware lane layouts the kernels rely on)
 * ---------------------------------------------------------------------------------------- */
/* out: DEVICE [11][64] floats; row k = op k applied to the lane index:
 * 0 quad_xor1, 1 quad_xor2, 2..5 quad_bcast<0..3>, 6 row_ror<1>, 7 row_ror<4>, 8 row_ror<8>,
 * 9 row_half_mirror, 10 wave_shr1 */
int clstm_debug_lane_ops(float* out);
/* C = A.B through the MFMA GEMM used by the hoisted products.  mode 0 "NN": A [R][K] row-major,
 * B [K][Cn] row-major; mode 1 "NT": A [R][K], B given as [Cn][K]; mode 2 "TN": A given as [K][R],
 * B [K][Cn] (split over K into nsplit slabs, reduced deterministically).  C [R][Cn] row-major.
 * Modes 10/11/12: the same three layouts through the bf16-input kernel (gemm_bf16.h). */
/* shader-clock timestamps of the last CTC launch's block 0 (HOST [16]): [0] start, [1..5] after phases A..E,
 * [6..15] sub-phase stamps of the short-line path (see scripts/gpu_ctcprof.py) */
int clstm_debug_ctc_cycles(long long* out_h);
int clstm_debug_gemm(int mode, const float* A, const float* B, float* C, int R, int Cn, int K, int nsplit);
/* how often this process has taken an optional fast path (HOST out).  The numbers are fixed (csrc/runtime.inc: enum PathCounter); which =
 *  0 / 1  persistent per-XCD forward / backward recurrence passes of a wide layer;
 *  2  W_x.x from bf16 operands (the lower layer's bf16 outputs, or a bf16 copy of the input frames);  3  x.d from the bf16 delta array;
 *  4  weight-gradient products from contraction-major bf16 operands (LDS transpose reads);  8  those of them that read their x rows from
 *     the layer below's bf16 outputs instead of a copy;  13  those that left the bias row to the recurrence's per-line sums;  14  those
 *     that computed the layer's x.d in the same launch (3 moves with it);
 *  5  the forward half as one launch (W_x producers + recurrence + softmax consumers, lstm_fwd_fused.h);
 *  6  persistent forward recurrences with the input projection folded in;
 *  9  persistent bf16 backward recurrences on the 32-cells-per-workgroup kernel;  11  persistent f32-grade (bf16 x 3) backward recurrences;
 *  10  fused updates that kept the packed parameter copies of a single narrow layer current;
 *  16 / 17 / 18  the recurrences batched over 16 lines on the MFMA (forward launch, backward launch, backward as one launch with the
 *     weight-gradient items: 17 moves with 18);
 *  22 / 23 / 15  the no-save forward passes of clstm_net_predict (per-line recurrence launches, fused forward launches, batched MFMA
 *     launches; the training counters 5 / 16 do not move for them);
 *  19  steps whose last reduction carried the next minibatch's ingest (clstm_net_train_step_next);  20  calls that found their minibatch
 *     declared by such a step;
 *  7  training steps whose gradient exchange was the peer-read all-reduce fused with the update (either form);  24  those of them that
 *     took the two-phase form;  12  replica consistency checks enqueued;
 *  25  lines normalised on the device (clstm_normalizer_run_*);  33  lines degraded on the device (clstm_degrader_run_*);
 *  26  backward passes whose top layer's recurrence workgroups computed the softmax layer's input deltas themselves, in front of
 *     their first step (lstm_xd_prologue.h), instead of a product launch of its own (experiment option xd_prologue=0);
 *  27  backward passes that took the producer form of the same instead (the default where narrow_plan admits it; xd_prologue=1: never): every recurrence workgroup
 *     computed only the 32 frames it visits first, helper workgroups of the launch the rest (26 does not move for them);
 *  28  score launches (clstm_ctc_score_batch / clstm_net_score): one per form a call launched -- the sum form for score_h, the
 *     max-plus form for vscore_h / path_h;
 *  29  beam-search launches (clstm_ctc_beam_batch / clstm_net_beam): one per call that had a line with frames;
 *  30  the same with a language model (clstm_ctc_beam_lm_batch / clstm_net_beam_lm); 29 does not move for them;
 *  31  edit-distance launches (clstm_edit_distance_batch / clstm_net_errors): one per call that had a pair;
 *  32  beam-search launches constrained to a lexicon (clstm_ctc_beam_lex_batch / clstm_net_beam_lex); 29 and 30 do not move for them;
 *  21  minibatches whose forward pass the batched kernel handed to the per-line kernels on the device (inputs outside [-255, 255];
 *     counted on the device: blocking).
 * Tests use it to make sure the path they mean to cover is the one that ran. */
int clstm_debug_path_count(int which, long long* out_h);
/* Experiment switches of the library (clstm_amd/csrc/dbgopt.h: the table of names and defaults, e.g. "gemm_stag", "bwd_c32",
 * "rec_x3", "pack_tiles"): tests compare the two sides bit for bit within one process.  A name not in the table is an error.
 * name NULL: forget every option.  Whole programs: environment CLSTM_DEBUG="name=value,...".  Not product settings. */
int clstm_debug_set_option(const char* name, int value);
/* (tests) set a device error word: which = 0 the outcome word of the persistent recurrences, 1 the count of weight-gradient
 * items that gave up waiting.  While either is non-zero clstm_net_update() applies nothing; the next synchronisation
 * point (clstm_synchronize, any *_h read-back) reports the error and clears the words. */
int clstm_debug_set_device_error(int which, int value);
/* Which lock-step kernel a wide layer's pass runs (csrc/runtime.inc: wide_plan, the one place that decides): host arithmetic, no net, no device.
 * shape (20 ints, HOST in): fwd, no, x_ni (the layer's inputs), ndir, bs, tmax, N (frames), kp, kp16 (padded contraction lengths of the
 *   pass: f32 rows, multiple of 64 / bf16 rows, multiple of 128), bf16 (precision mode 2), x3 (backward: the x3 kernel asked for and its
 *   weights packed), fx_mode (forward: option fuse_wx where the folded input projection has its operands, else 0), ncu, xcd_on
 *   (CLSTM_XCD_REC), xcd_failed (a placement check has failed in this process), c32_on (option bwd_c32), sbf (the pass writes bf16 source
 *   rows), sbf_ld, lds, ldh (row strides of the bf16 source, f32 source and output rows).
 * plan (14 ints, HOST out): kernel, param, fullk -- the persistent kernel tried first, 0 none, 1 xcd_fwd_f32, 2 xcd_fwd_bf16<MT>,
 *   3 xcd_fwd_bf16_fx<NGX>, 4 xcd_bwd_x3, 5 xcd_bwd_f32, 6 xcd_bwd_bf16_c32<EPT, FULLK>, 7 xcd_bwd_bf16<MT>; nzb, zb_per (line blocks, and
 *   how many one launch walks), launches (of what runs if every placement check holds: chunks, or tmax per-step launches), lds_bytes;
 *   step_kernel, step_param -- what runs per time step otherwise: 8 wide_fwd_step<MT>, 9 wide_fwd_step16_bf16, 10 wide_bwd_step,
 *   11 wide_bwd_step16_bf16, 0 none (behind kernel 3 the caller runs the hoisted product and asks again with fx_mode 0); step_grid[3];
 *   moves (bit c: a successful persistent pass moves clstm_debug_path_count(c)); fx_ngx (the folded projection was asked for). */
int clstm_debug_wide_plan(const int* shape, int* plan);
/* What the net holds, as 8 ints; host only: enqueues nothing, touches no device memory.
 *   out: bs, N (frames), then the record (csrc/net.inc: Net::Holds): batch (0 none, 1 the current minibatch, 2 a declared next one whose outputs
 *   do not exist), training_buffers (1 the buffers of a training pass, 0 predict's forward-only geometry), forward (0 no pass of this minibatch
 *   yet, 1 one that saved what a backward pass needs, 2 predict's no-save pass), frames (0 nowhere, 1 in the input block, 2 also in layer 0's
 *   source rows), offsets_sent (the line offsets are on the device), dx0 (a backward pass of this minibatch has written the input deltas). */
int clstm_debug_net_holds(clstm_net* net, int* out);
/* Which kernels a narrow (register-resident, nhidden <= 128) layer's pass runs, and in which launches (csrc/runtime.inc: narrow_plan, the one
 * place that decides): host arithmetic, no net, no device.
 * shape (30 ints, HOST in): pass (0 forward with save, 1 forward without save, 2 backward), no, ni, ndir; nlayers, first, top (this layer is
 *   the first / the top layer of the net); bs, tmax, N (frames), nc (classes); ldh, lds, ldx (row strides of the output, source and input
 *   rows), h_cap, d_cap (capacities of the output and delta buffers in floats: the 32-bit offset checks); wk (the fused forward's weights
 *   are packed), wk_njp, w1k_kps; overlap, bf16_gemm, strict_f32; dw_x3, split_terms (options, read at net creation); fwd_mfma (read by
 *   forward passes), bwd_mfma, bwd_mfma_fused, xd_prologue (by backward passes); ncu, emu (the host emulator build).
 * plan (11 ints, HOST out): nk4, ku, waves -- the class (nk4 0: none, the layer is wide); fwd -- forward family: 1 one workgroup per line,
 *   2 the fused forward launch, 3 batched over 16 lines on the MFMA; saves -- it runs its saving form; overlapped -- the backward family
 *   has the chunked weight-gradient items in or behind its launch; bwd -- launch form: 1 lstm_bwd_kernel, 2 that followed by
 *   gemm_dw_kernel, 3 lstm_bwd_xd_kernel (the x.d prologue) followed by gemm_dw_kernel, 4 one lstm_bwd_dw_kernel launch, 5 MFMA rows alone,
 *   6 MFMA rows followed by gemm_dw_kernel, 7 MFMA rows and items as one launch; terms -- split-term instantiation 3 / 2 / 0 (f32 MFMA);
 *   dwx -- the softmax layer's W.d slabs ride the launch; xd -- x.d form 0 (a launch of its own) / 1 (whole prologue) / 2 (producers);
 *   moves (bit c: the pass moves clstm_debug_path_count(c)).  Forward passes leave overlapped .. xd zero, backward passes fwd and saves. */
int clstm_debug_narrow_plan(const int* shape, int* plan);
/* Which kernels the matrix products around a layer's recurrence run -- the input projection W_x.x, the softmax layer's logits, its W.d and x.d,
 * the layer's weight gradient and its input deltas -- with which tile, rows and split-K slabs, and what the pass writes for them
 * (csrc/runtime.inc: product_plan, the one place that decides): host arithmetic, no net, no device.
 * shape (35 ints, HOST in): pass (0 forward, 1 backward); ni, no, ndir, wide (lock-step layer); first, top, nlayers; bwd_exact (the padded bf16
 *   backward rows are exactly 4 no: no % 32 == 0), kp16f_is_no (no % 128 == 0); N (frames), bs (lines); nclasses, sm_ni (inputs of the softmax
 *   layer); precision (clstm_net_set_gemm_precision), gemm_x3_on, split_terms (options, read at net creation), strict
 *   (clstm_net_set_strict_f32); gemm_b16mc, gemm_stag, pack_tiles, fuse_wx (options, read per pass); ncu, want_dx0
 *   (clstm_net_enable_input_deltas); fwd_family, overlapped, dwx, xd (the layer's narrow plan: fwd / overlapped / dwx / xd; a wide layer: 0),
 *   dw_slabs_per_dir, dwx_nslabs (slab counts of the Overlapped items' tables); the facts of earlier launches: below_hbf (the layer below ran
 *   its persistent bf16 forward kernel and left bf16 outputs), fwd_sbf (this layer's forward pass ran persistent and wrote bf16 source rows),
 *   bwd_persistent (its backward recurrence ran persistent), packs, above_packs (the bf16 packs of W_x exist for this layer / the layer above).
 * plan (39 ints, HOST out): six products of four ints each -- kernel, tile (rows of an output tile: 64 / 128 / 192 / 256, 0 the fused
 *   softmax's own), rows (it is launched with), slabs (split-K slabs per direction) -- in the order wx, logits (forward), sm_wd, sm_xd, dw, dx
 *   (backward); kernel: 0 none (part of a recurrence launch), 1 gemm_f32, 2 gemm_bf16, 3 gemm_b16kk, 4 gemm_b16mc, 5 gemm_dw_dx, 6 gemm_x3,
 *   7 gemm_x3_big, 8 gemm_x3_pair, 9 gemm_f32_pair, 10 softmax_fwd.  Then merged (dw and dx are one launch), bias_out (the bias row is laid
 *   outside dw); dw16_rows, dw16_tile, x_external (rows and tile height of the bf16-source weight gradient and whether the x block fills whole
 *   tiles of it: functions of the shape and the mode alone, equal in both passes whatever the facts say); a2_rows (rows the weight gradient
 *   reads from the layer below's bf16 outputs, 0: copied into the source rows); x_copy (wx reads a bf16 copy of the input frames); fx_mode
 *   (fuse_wx where the folded input projection has its operands, else 0: clstm_debug_wide_plan's fx_mode); tiled_pack (the repack is
 *   k_pack_wide_tiles); stag, terms; writes (bit 0 Sbf, 1 Hbf, 2 Dbf and dbias), skips (f32 stores the persistent kernel may skip: bit 0 H,
 *   1 the h columns of S, 2 D), needs (built first: bit 0 the f32 source rows, 1 the f32 deltas, 2 the f32 outputs of the layer below);
 *   moves (bit c: the pass moves clstm_debug_path_count(c); 2 where wx is launched, 3, 4, 8, 13, 14 by the backward pass). */
int clstm_debug_product_plan(const int* shape, int* plan);
/* Which path of the alignment kernel every line of a minibatch takes (csrc/ctc.h: ctc_batch_plan, ctc_line_plan, ctc_scores_in_lds -- the
 * functions clstm_ctc_align_batch and the kernel's workgroups themselves decide with): host arithmetic, no net, no device.  Arguments as
 * clstm_ctc_align_batch's.  A line's path depends on the other lines of its minibatch through tile and smax.
 * batch_plan_h (4 ints, HOST out): tile (frames per LDS tile), smax (the most states of a line, capped at 2048), ncp (LDS row stride of the
 *   class tile: nc | 1), LDS bytes of the launch.
 * line_plan_h (13 ints per line, in line order, HOST out):
 *   0 T, 1 S, 2 nu (distinct classes among the line's states);
 *   3 form: 0 short line (every phase in one LDS region), 1 tiled (lattices in memory, phases A and E tile by tile), 2 huge (more than
 *     2048 states: per-state arrays in memory), 3 none (no frames or no states: nothing is written);
 *   4 recursion: 0 one wave per direction, one state per lane (S <= 64), 1 two states per lane (S <= 128), 2 / 3 groups of 256 lanes
 *     holding up to 2 / up to 8 states each, 4 rounds over the label axis;
 *   short lines (0 otherwise): 5 flat (posteriors held in registers across the classification, copied flat into LDS), 6 lds_lat (both
 *     lattices of the recursion in LDS), 7 lm_lds (the recursion reads its match scores from LDS), 8 lanemap (phases C / D with lane =
 *     state);
 *   tiled and huge lines (0 otherwise): 9 flat_stage (posterior tiles copied flat), 10 c_in_regs (phase C keeps the cells in registers
 *     between its passes), 11 d_per_state (phase D one thread per state), 12 ntiles (tiles phases A and E walk).
 * Tests use it to make sure the path they mean to cover is the one that runs (tests/test_ctc_path_sweep.py). */
int clstm_debug_ctc_plan(int nc, const int* line_off_h, const int* states_h, const int* state_off_h, int bs, int* batch_plan_h,
                         int* line_plan_h);
/* Which form a pair of the edit-distance kernel takes (csrc/edit_distance.h: edit_plan -- the function the host sizes the launch with and
 * the pair's wave addresses with): host arithmetic, no net, no device.  la, lb: hypothesis and reference length (for clstm_net_errors la is
 * the line's frames); want_script: anything beyond dist_h is asked for.
 * plan (5 ints, HOST out): 0 strips of 64 reference columns (0: an empty reference); 1 directions: 0 none (distances only, or an empty
 *   side), 1 in the wave's LDS carve, 2 in the workspace; 2 the edge column between strips: 0 none (one strip), 1 LDS (la < 1024), 2
 *   workspace; 3 direction words per column (ceil(la / 16) made odd); 4 words of the wave's LDS carve (at most 4096). */
int clstm_debug_edit_plan(int la, int lb, int want_script, int* plan);
/* How many workgroups the alignment launch gives every line that splits (csrc/ctc.h: ctc_nsplit): host arithmetic, no net, no device when
 * ncu > 0.  bs: lines of the minibatch; ncu: CUs (0: the current device's; the emulator's stand-in).  *nsplit_h (HOST out): 4, 2 or 1 --
 * the largest with bs * n <= ncu, or what the experiment option ctc_split (1, 2, 4) forces.  A line splits where clstm_debug_ctc_plan
 * answers form 0 and lm_lds 1 (match scores and both lattices in LDS); every other line keeps one workgroup, and a minibatch without such
 * a line, or whose outputs overlap its posteriors, is launched with one workgroup per line whatever this answers. */
int clstm_debug_ctc_split(int bs, int ncu, int* nsplit_h);
/* range_h[0 .. 1] (HOST out): the frames [lo, hi) that part k of the n workgroups of a line of T frames emits (csrc/ctc.h:
 * ctc_part_frames, the function the kernel calls). */
int clstm_debug_ctc_part_frames(int T, int n, int k, int* range_h);
/* clstm_debug_ctc_cycles for part `part` (0 .. 3) of line 0's workgroups (part 0: the same stamps). */
int clstm_debug_ctc_cycles_part(int part, long long* out_h);

#ifdef __cplusplus
}
#endif
#endif /* CLSTM_ABI_H_ */
