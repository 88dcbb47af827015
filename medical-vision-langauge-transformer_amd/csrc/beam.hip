// Beam search bookkeeping on the device: BeamScorer.process of decode.py (HF transformers 4.16 BeamSearchScorer.process) and the
// three lines beam_search runs behind it, as one launch (mvlt_beam_step, contract in include/mvlt_hip.h).
#include "common.h"

namespace {

constexpr int BS_MAXB = 8, BS_MAXC = 16, BS_THREADS = 256;
constexpr int BS_STAGE = 8192;          // int32 words of LDS that stage a sample's num_beams x max_length rows (seq, then the slot table)

struct BeamStepDev {
    int G, nb, n_cand, src_beams, max_length, has_eos;
    long eos, pad, mask;
    const float* cand_score; const int* cand_beam; const int* cand_tok;
    double* hyp_score; int* hyp_len; int* hyp_tokens; int* n_hyp; double* worst; int* done;
    int* seq; int* slot; long ld_slot;
    int64_t* col; int* past; int* ticket; int64_t* alive;
    float* beam_scores; int64_t* new_ids; int* beam_idx;
    int* cand_log;
};

// One workgroup per sample.  Lane 0 walks the candidates in rank order and keeps the pool's scalars (scores, lengths, count, worst)
// exactly as BeamHypotheses.add does, in f64; what the walk decides about token ROWS goes into a short list in LDS -- "the staged
// row `src` becomes pool entry `dst`, then entry `evict` is deleted and the later ones move up" -- that all lanes carry out.
// The sample's seq rows are staged in LDS before anything is written: the pool copies read the rows of BEFORE this step, and the
// permutation by parent happens in place.  The slot table goes through the same LDS area afterwards.
// Every workgroup reads *col before it draws its ticket, and *col is written only after all tickets are drawn.
__global__ __launch_bounds__(BS_THREADS) void beam_step_kernel(const BeamStepDev p) {
    __shared__ int s_stage[BS_STAGE];
    __shared__ float s_keep_score[BS_MAXB];
    __shared__ int s_keep_tok[BS_MAXB], s_keep_par[BS_MAXB];
    __shared__ int s_op_src[BS_MAXB], s_op_dst[BS_MAXB], s_op_evict[BS_MAXB];
    __shared__ double s_hs[BS_MAXB + 1];
    __shared__ int s_hl[BS_MAXB + 1];
    __shared__ int s_nops, s_n0;
    const int g = blockIdx.x, tid = threadIdx.x, nb = p.nb, ml = p.max_length;
    const long col = p.col[0];
    const bool in_range = col >= 0 && col < ml;          // (a caller that steps past max_length gets no write outside the buffers)
    const int row0 = g * nb;
    const float* c_score = p.cand_score + (long)g * p.n_cand;
    const int* c_beam = p.cand_beam + (long)g * p.n_cand;
    const int* c_tok = p.cand_tok + (long)g * p.n_cand;
    if (in_range && p.cand_log) {
        int* lg = p.cand_log + ((long)col * p.G + g) * 3 * p.n_cand;
        for (int i = tid; i < p.n_cand; i += BS_THREADS) {
            lg[i] = __float_as_int(c_score[i]);
            lg[p.n_cand + i] = c_beam[i];
            lg[2 * p.n_cand + i] = c_tok[i];
        }
    }
    const bool was_done = in_range ? p.done[g] != 0 : true;
    if (in_range && was_done) {
        for (int k = tid; k < nb; k += BS_THREADS) {
            p.beam_scores[row0 + k] = 0.f;
            p.new_ids[2L * (row0 + k)] = p.pad;
            p.new_ids[2L * (row0 + k) + 1] = p.mask;
            p.beam_idx[row0 + k] = 0;
        }
    }
    if (in_range && !was_done) {          // (uniform over the workgroup: the barriers below are safe)
        const int L = col < 1 ? 1 : (int)col;          // length of what the scorer is handed: [[mask_id]] at step 0
        for (int i = tid; i < nb * ml; i += BS_THREADS) s_stage[i] = p.seq[(long)row0 * ml + i];
        if (tid == 0) {
            double* hs = s_hs;
            int* hl = s_hl;
            int n = p.n_hyp[g];
            n = n < 0 ? 0 : (n > nb ? nb : n);          // (a pool count the caller never initialised must not index outside the pool)
            double worst = p.worst[g];
            double* gs = p.hyp_score + (long)g * (nb + 1);
            int* gl = p.hyp_len + (long)g * (nb + 1);
            s_n0 = n;
            for (int i = 0; i < n; ++i) { hs[i] = gs[i]; hl[i] = gl[i]; }
            int kept = 0, nops = 0;
            for (int rank = 0; rank < p.n_cand && kept < nb; ++rank) {
                const float sc = c_score[rank];
                const int tok = c_tok[rank];
                int par = c_beam[rank];
                par = par < 0 ? 0 : (par >= p.src_beams ? p.src_beams - 1 : par);
                if (p.has_eos && (long)tok == p.eos) {
                    if (rank >= nb) continue;
                    const double score = (double)sc / (double)L;
                    if (n < nb || score > worst) {
                        hs[n] = score; hl[n] = L;
                        s_op_src[nops] = par; s_op_dst[nops] = n; s_op_evict[nops] = -1;
                        ++n;
                        if (n > nb) {          // drop the lowest (score, insertion index); worst = the second lowest score
                            int v = 0;
                            for (int i = 1; i < n; ++i) if (hs[i] < hs[v]) v = i;
                            double second = 0.0; bool have = false;
                            for (int i = 0; i < n; ++i) if (i != v && (!have || hs[i] < second)) { second = hs[i]; have = true; }
                            for (int i = v; i + 1 < n; ++i) { hs[i] = hs[i + 1]; hl[i] = hl[i + 1]; }
                            --n;
                            worst = second;
                            s_op_evict[nops] = v;
                        } else {
                            worst = score < worst ? score : worst;
                        }
                        ++nops;
                    }
                } else {
                    s_keep_score[kept] = sc; s_keep_tok[kept] = tok; s_keep_par[kept] = par;
                    ++kept;
                }
            }
            for (; kept < nb; ++kept) { s_keep_score[kept] = 0.f; s_keep_tok[kept] = (int)p.pad; s_keep_par[kept] = 0; }
            for (int i = 0; i < n; ++i) { gs[i] = hs[i]; gl[i] = hl[i]; }
            p.n_hyp[g] = n;
            p.worst[g] = worst;
            const bool done = n >= nb && worst >= (double)c_score[0] / (double)L;
            if (done) p.done[g] = 1;
            s_nops = nops;
            if (!done) atomicMax(reinterpret_cast<unsigned long long*>(p.alive + col), 1ULL);
        }
        __syncthreads();
        // the pool's token rows, op by op (at most num_beams of them)
        int* pool = p.hyp_tokens + (long)g * (nb + 1) * ml;
        int n_rows = s_n0;
        for (int o = 0; o < s_nops; ++o) {
            const int src = s_op_src[o], dst = s_op_dst[o], ev = s_op_evict[o];
            for (int c = tid; c < L; c += BS_THREADS) pool[(long)dst * ml + c] = col < 1 ? (int)p.mask : s_stage[src * ml + c];
            n_rows = dst + 1;
            if (ev >= 0) {          // a thread owns a column: the rows move up in order, no two threads touch one cell
                for (int c = tid; c < ml; c += BS_THREADS)
                    for (int i = ev; i + 1 < n_rows; ++i) pool[(long)i * ml + c] = pool[(long)(i + 1) * ml + c];
                --n_rows;
            }
            __syncthreads();
        }
        // live beams: scores, ids of the next forward, parents; seq rows permuted by parent with the token appended
        for (int k = tid; k < nb; k += BS_THREADS) {
            p.beam_scores[row0 + k] = s_keep_score[k];
            p.new_ids[2L * (row0 + k)] = s_keep_tok[k];
            p.new_ids[2L * (row0 + k) + 1] = p.mask;
            p.beam_idx[row0 + k] = row0 + s_keep_par[k];
        }
        for (int i = tid; i < nb * ml; i += BS_THREADS) {
            const int k = i / ml, c = i - k * ml;
            p.seq[(long)row0 * ml + i] = c == col ? s_keep_tok[k] : s_stage[s_keep_par[k] * ml + c];
        }
        __syncthreads();
        for (int i = tid; i < nb * ml; i += BS_THREADS) {
            const int k = i / ml, c = i - k * ml;
            s_stage[i] = p.slot[(long)(row0 + k) * p.ld_slot + c];
        }
        __syncthreads();
        for (int i = tid; i < nb * ml; i += BS_THREADS) {
            const int k = i / ml, c = i - k * ml;
            p.slot[(long)(row0 + k) * p.ld_slot + c] = c == col ? k : s_stage[s_keep_par[k] * ml + c];
        }
    }
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        if (atomicAdd(p.ticket, 1) == p.G - 1) {
            *p.ticket = 0;
            if (in_range) {
                p.col[0] = col + 1;
                if (p.past) p.past[0] += 1;
            }
        }
    }
}

}  // namespace

extern "C" int mvlt_beam_step(const MvltBeamStep* b, void* stream) {
    MVLT_CHECK(b, MVLT_ERR_ARG);
    MVLT_CHECK(b->cand_score && b->cand_beam && b->cand_tok && b->hyp_score && b->hyp_len && b->hyp_tokens && b->n_hyp && b->worst && b->done,
               MVLT_ERR_ARG);
    MVLT_CHECK(b->seq && b->slot && b->col && b->ticket && b->alive && b->beam_scores && b->new_ids && b->beam_idx, MVLT_ERR_ARG);
    MVLT_CHECK(b->G >= 1 && b->num_beams >= 1 && b->n_cand >= b->num_beams && b->max_length >= 1 && b->ld_slot >= b->max_length, MVLT_ERR_ARG);
    MVLT_CHECK(b->src_beams == 1 || b->src_beams == b->num_beams, MVLT_ERR_ARG);
    MVLT_CHECK(b->num_beams <= BS_MAXB && b->n_cand <= BS_MAXC, MVLT_ERR_UNSUPPORTED);
    MVLT_CHECK((long)b->num_beams * b->max_length <= BS_STAGE, MVLT_ERR_UNSUPPORTED);
    const BeamStepDev d{b->G, b->num_beams, b->n_cand, b->src_beams, b->max_length, b->has_eos, (long)b->eos_id, (long)b->pad_id, (long)b->mask_id,
                        b->cand_score, b->cand_beam, b->cand_tok, b->hyp_score, b->hyp_len, b->hyp_tokens, b->n_hyp, b->worst, b->done,
                        b->seq, b->slot, (long)b->ld_slot, b->col, b->past, b->ticket, b->alive, b->beam_scores, b->new_ids, b->beam_idx, b->cand_log};
    hipLaunchKernelGGL(beam_step_kernel, dim3(b->G), dim3(BS_THREADS), 0, reinterpret_cast<hipStream_t>(stream), d);
    MVLT_LAUNCH_CHECK();
    return MVLT_OK;
}
