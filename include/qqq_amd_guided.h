/*
 * qqq_amd_guided.h -- C-ABI of the two device ops behind guided decoding (exported by libqqq_amd.so, beside include/qqq_amd.h and the
 * other per-feature headers): a completion follows a deterministic automaton over token ids that lives in device memory.  qqq_fsm_mask runs in FRONT of a
 * sampler and leaves only the tokens the row's state allows; qqq_fsm_advance runs BEHIND qqq_sample_advance (include/qqq_amd_step.h) and
 * moves the state on over the token just drawn.  Both sit inside a decode loop's captured step, so no token leaves the device between
 * two syncs.  All of it is integer and bit work.
 *
 * The automaton, states 0 ... n_states - 1, in CSR form (qqq_amd/guided.py builds and validates it):
 *   offsets       int32 [n_states + 1]   state s owns the edges lo(s) ... hi(s) - 1
 *   tokens        int32 [n_edges]        an edge's token, strictly ascending inside a state
 *   next          int32 [n_edges]        an edge's target state
 *   accept        int32 [n_states]       non-zero: the row's eos may be drawn in this state
 *   lo(s) = clamp(offsets[s], 0, n_edges), hi(s) = max(lo(s), clamp(offsets[s + 1], 0, n_edges)): both offsets are clamped into
 *   [0, n_edges], and an end below its begin is an empty edge list.  A state with lo(s) == hi(s) is TERMINAL.  tokens and next may be
 *   NULL exactly when n_edges == 0.
 *
 * qqq_fsm_mask
 *   logits        fp16 [rows, vocab], row stride ld elements (ld >= vocab), 2-byte aligned, rewritten in place
 *   state         int32 [rows]   the rows' states
 *   eos           int32 [rows] or NULL   the row's eos id, -1 for none
 *   remaining     int32 [rows] or NULL   a decode loop's budgets: a row with 0 is idle
 *   Per row r with s = state[r]: the row is left untouched when s is outside [0, n_states), and when remaining is given and
 *   remaining[r] == 0.  Otherwise every column v in [0, vocab) becomes fp16 -inf (0xFC00), except
 *     - the columns tokens[e] for lo(s) <= e < hi(s), and
 *     - eos[r], if eos is given, accept[s] != 0 and eos[r] lies in [0, vocab).
 *   An allowed column keeps its bits, NaN and -inf included; so do the columns vocab ... ld - 1.  The op never reads the logits: it
 *   writes the disallowed columns and steps around the others.
 *   A row's columns are split over several workgroups, each of which finds its part of the state's edge list by a search over
 *   tokens[lo(s) ... hi(s)) that presumes the ascending order; the split depends on (rows, vocab) alone.  A token is range-checked
 *   against the workgroup's columns before it is used, so a table that breaks the rules above may give a wrong mask, never an access
 *   outside the arrays.
 *
 * qqq_fsm_advance
 *   out           int64 [rows, out_stride]   the rows' emitted tokens;  n_out  int32 [rows]  their counts
 *   n_fsm         int32 [rows]   the count up to which the row's state has been advanced, updated in place
 *   state         int32 [rows]   updated in place;  eos  int32 [rows] or NULL
 *   ids, pos, slots   int64 [rows];  remaining  int32 [rows]: the row state to retire
 *   Per row r: if n_fsm[r] >= n_out[r] the row writes nothing at all.  Otherwise, for i = max(n_fsm[r], 0) ... n_out[r] - 1 in order
 *   while i < out_stride, with t = out[r, i] and s = state[r]:
 *     1. s outside [0, n_states): nothing happens;
 *     2. else, if an edge e of s has tokens[e] == t (a search over the ascending tokens), with s' = next[e]:
 *        s' outside [0, n_states): state[r] = -2 and the row retires; else state[r] = s', and the row retires if s' is terminal;
 *     3. else, if accept[s] != 0, eos is given and t == eos[r] >= 0: the state stays as it is (the sampler has retired the row);
 *     4. else state[r] = -2 and the row retires.
 *   Finally n_fsm[r] = n_out[r].  "Retires" is include/qqq_amd_step.h's: ids[r] = 0, pos[r] = slots[r] = -1, remaining[r] = 0.
 *   State -2 records a token outside the automaton: behind qqq_fsm_mask that is only possible when every allowed logit was -inf or NaN.
 *   A caller sets n_fsm = 0 (with n_out = 0) and state = the state behind the first token when it admits a sequence, and -1 for a row
 *   that follows no automaton.
 *
 * One launch each; the launch size depends on (rows, vocab) / on rows alone and nothing is read on the host, so a captured graph replays
 * with other contents of every array -- another automaton in the same buffers included.  No workspace.  Conventions are those of
 * include/qqq_amd.h: work only ENQUEUED on `stream` (safe under hipGraph capture), no allocation, no state.  Return codes QQQ_OK /
 * QQQ_ERR_ARG / QQQ_ERR_HIP with a message in qqq_amd_last_error() that begins with the entry's name; bad arguments are rejected before
 * any launch.  rows == 0 is a no-op (NULL pointers allowed).
 * Limits: 0 <= rows <= 65535, 1 <= vocab <= 262144, ld >= vocab, n_states >= 1, n_edges >= 0, out_stride >= 1.
 * Alignment: logits 2 bytes; out, ids, pos and slots 8 bytes; everything else 4 bytes.
 */
#ifndef QQQ_AMD_GUIDED_H_
#define QQQ_AMD_GUIDED_H_

#include "qqq_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int qqq_fsm_mask(void* logits, int ld, const void* state, const void* eos /* may be NULL */, const void* remaining /* may be NULL */,
                 const void* offsets, const void* tokens /* NULL iff n_edges == 0 */, const void* accept, int n_states, int n_edges,
                 int rows, int vocab, int dev, void* stream);

int qqq_fsm_advance(const void* out, int out_stride, const void* n_out, void* n_fsm, void* state, const void* eos /* may be NULL */,
                    const void* offsets, const void* tokens /* NULL iff n_edges == 0 */, const void* next /* NULL iff n_edges == 0 */,
                    const void* accept, int n_states, int n_edges, void* ids, void* pos, void* slots, void* remaining, int rows, int dev,
                    void* stream);

#ifdef __cplusplus
}
#endif

#endif /* QQQ_AMD_GUIDED_H_ */
