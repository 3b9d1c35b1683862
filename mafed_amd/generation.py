"""Generation for ``VLPythiaForCausalLM``: greedy search, beam search, sampling and candidate scoring, the KV-cached decode step, its cache and the
captured-graph decode.
``GenerationMixin`` is a base class of the model (mafed_amd/model.py, which this module does not import): it uses the model's engine
forward and its pieces (mafed_amd/engine.py: layer body, projector, parameter readiness, final LayerNorm + head), parameter records and rotary tables, and the state ``fused_decode`` / ``beam_trace`` / ``_decode_graphs`` its ``__init__`` declares."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional, Tuple

import torch

from mafed_amd import ops


@dataclass
class BeamSearchOutput:
    """``generate(..., return_dict_in_generate=True)``: the fields of transformers' GenerateBeamDecoderOnlyOutput that are produced."""

    sequences: torch.Tensor
    sequences_scores: Optional[torch.Tensor] = None


def _eos_cut(gen: torch.Tensor, eos_token_id) -> int:
    """HF leaves the loop as soon as every row has finished: of the tokens ``gen`` [R, n] -> how many the slowest row needed, up to and
    including its first eos.  The one host synchronisation of the greedy and the sampled paths."""
    if eos_token_id is None:
        return gen.shape[1]
    done = (gen == eos_token_id).to(torch.int64).cumsum(1).clamp_(max=1)       # 1 from the first eos on
    first = (done.shape[1] - done.sum(1)) + done[:, -1]                        # tokens up to and including the first eos
    return int(first.max().clamp_(max=gen.shape[1]))


def _rows(x: torch.Tensor, n: int) -> torch.Tensor:
    """Every row of ``x`` n times in a row (HF's ``expand_inputs_for_generation`` order)."""
    return x.repeat_interleave(n, 0) if n > 1 else x


class _GreedyPick:
    """A pick object is what differs between greedy, sampled and beam decoding; ``GenerationMixin._decode`` is the loop around it.  It says
    into how many ``rows`` a prompt expands, draws the next tokens [B * rows] from the step's logits when called with (logits, step) --
    step 0 of the cached loop hands it the prefill's one row per prompt --, sees the cache once after the prefill (``start``) and before
    every cached step (``before_step``), names the tokens of the steps so far for the recompute loop (``drawn``) and assembles the result
    (``result``, the one host synchronisation).  For the captured graph: ``key`` tells two captures apart (None: cannot be captured),
    ``reset`` forgets the draws from inside the captured body, ``inputs`` are the device words a replay reads.
    This one is HF ``greedy_search``; it owns the ``unfinished`` flags, the drawn tokens and, if wanted, every step's logits."""

    rows, key, inputs = 1, (), ()

    def __init__(self, R: int, dev, eos_token_id, pad_token_id, want_steps: bool = False, flags: bool = True):
        self.R, self.dev, self.eos, self.pad, self.want_steps = R, dev, eos_token_id, pad_token_id, want_steps
        self.unfinished = torch.ones(R, dtype=torch.int64, device=dev) if flags else None
        self.tokens, self.steps, self.logprobs = [], [], []

    def reset(self) -> None:
        self.unfinished = torch.ones_like(self.unfinished)
        self.tokens, self.steps, self.logprobs = [], [], []

    def start(self, cache: "_DecodeCache") -> None:
        pass

    def before_step(self, cache: "_DecodeCache") -> None:
        pass

    def __call__(self, logits: torch.Tensor, t: int) -> torch.Tensor:
        nxt = logits.float().argmax(dim=-1)   # the token rule: argmax of the last position, finished rows emit ``pad_token_id``
        if self.eos is not None:
            nxt = nxt * self.unfinished + self.pad * (1 - self.unfinished)
            self.unfinished = self.unfinished * (nxt != self.eos).to(torch.int64)
        return self._keep(nxt, logits)

    def _keep(self, nxt: torch.Tensor, logits: torch.Tensor) -> torch.Tensor:
        self.tokens.append(nxt)
        if self.want_steps:
            self.steps.append(logits.float())
        return nxt

    def drawn(self, t: int) -> torch.Tensor:
        return torch.stack(self.tokens, dim=1)

    def result(self, ids: torch.Tensor) -> Tuple[Optional[torch.Tensor], ...]:
        """-> (sequences [B * rows, T + n_keep], the kept steps' logits [n_keep, B * rows, V] or None, the kept draws' log-probabilities
        [B * rows, n_keep] or None): all three cut at ``_eos_cut``."""
        gen = torch.stack(self.tokens, dim=1)
        n_keep = _eos_cut(gen, self.eos)
        return (torch.cat([_rows(ids, self.rows), gen[:, :n_keep]], dim=1), torch.stack(self.steps[:n_keep], dim=0) if self.want_steps else None,
                torch.stack(self.logprobs, dim=1)[:, :n_keep] if self.logprobs else None)


class _SampledPick(_GreedyPick):
    """HF ``sample`` for n = ``rows`` sequences per prompt, every draw one launch of ``ops.sample_token``: beside the greedy state it owns the
    seed's device word and, if wanted, the drawn tokens' log-probabilities.  Over the cache the n samples of a prompt share its prefix:
    each keeps its slot for good (an identity ancestry table), and step 0 draws all n from the prompt's one logits row."""

    def __init__(self, R: int, dev, eos_token_id, pad_token_id, warp, n: int, seed: int, want_steps: bool = False, want_logprobs: bool = False):
        super().__init__(R, dev, eos_token_id, pad_token_id, want_steps, flags=eos_token_id is not None)
        self.rows, self.warp, self.key, self.want_logprobs = n, warp, ("sample",) + warp, want_logprobs
        self.seed = ops.seed_word(seed, dev)
        self.inputs = (self.seed,)   # a replay of the captured steps reads the seed from this word: a new seed needs no new capture

    def reset(self) -> None:
        if self.unfinished is not None:
            self.unfinished.fill_(1)   # the draws update it in place: one buffer, reset at the head of every replay
        self.tokens, self.steps, self.logprobs = [], [], []

    def start(self, cache: "_DecodeCache") -> None:
        if self.rows > 1:
            if not cache.prerot:
                raise NotImplementedError("sampling n > 1 over the shared prefix needs the pre-rotated cache (rotary dims % 16 == 0, head size 64 / 128 / 256)")
            # every sample keeps its own slot for good: the ancestry table of the beam attention is the identity
            cache.anc = torch.arange(self.R, dtype=torch.int32, device=self.dev)[:, None].expand(self.R, cache.cap).contiguous()

    def __call__(self, logits: torch.Tensor, t: int) -> torch.Tensor:
        if logits.shape[0] != self.R:
            logits = logits.repeat_interleave(self.rows, 0)   # the prompt's one row, named n times (counters b * n + j)
        lp = None
        if self.want_logprobs:
            lp = torch.empty(self.R, dtype=torch.float32, device=self.dev)
            self.logprobs.append(lp)
        temperature, top_k, top_p, min_p = self.warp   # the token rule, one launch; ``unfinished`` is updated in place
        return self._keep(ops.sample_token(logits, temperature, top_k, top_p, min_p, seed=self.seed, step=t, unfinished=self.unfinished, eos_token_id=self.eos,
                                           pad_token_id=0 if self.pad is None else self.pad, logprob=lp), logits)


class _BeamPick:
    """Beam search with k = ``rows`` beams per prompt (generate(num_beams=k)); every decision on the device (csrc/beam.hip; the beams'
    attention is csrc/attn_decode_beam.hip), one host synchronisation in ``result``.
    Per step: mafed_beam_candidates (top 2k of log_softmax + running score per sample) and mafed_beam_update (finished set,
    continuing beams, early stopping, ancestry / history rewrite) between two copies of the state, ``cur`` naming the live one.  The loop
    runs to max_new_tokens like the greedy path: a sample whose result is final stops changing (HF leaves the loop once every sample is
    such), and the output is cut at the end."""

    key, want_steps = None, False

    def __init__(self, B: int, dev, eos_token_id, pad_token_id, k: int, cap: int, length_penalty: float, early_stopping, nrs: int,
                 return_dict: bool, trace: Optional[list]):
        eos, pad = -1 if eos_token_id is None else int(eos_token_id), 0 if pad_token_id is None else int(pad_token_id)
        self.B, self.rows, self.dev, self.nrs, self.return_dict, self.trace = B, k, dev, nrs, return_dict, trace
        self.args = (cap, eos, pad, {False: 0, True: 1, "never": 2}[early_stopping], length_penalty)
        BK = B * k
        i32, i64, f32 = torch.int32, torch.int64, torch.float32
        self.cand = (torch.empty((B, 2 * k), dtype=f32, device=dev), torch.empty((B, 2 * k), dtype=i64, device=dev),
                     torch.empty((B, 2 * k), dtype=i32, device=dev))
        self.run_score = torch.zeros(BK, dtype=f32, device=dev)
        self.anc = [torch.zeros((BK, cap), dtype=i32, device=dev) for _ in range(2)]
        self.hist = [torch.zeros((BK, cap), dtype=i64, device=dev) for _ in range(2)]
        self.fin_tok = [torch.full((B, k, cap), pad, dtype=i64, device=dev) for _ in range(2)]
        self.fin_score = [torch.full((B, k), -1e9, dtype=f32, device=dev) for _ in range(2)]
        self.fin_len = [torch.zeros((B, k), dtype=i32, device=dev) for _ in range(2)]
        self.done = torch.zeros(B, dtype=i32, device=dev)
        self.next_tok = torch.zeros(BK, dtype=i64, device=dev)
        self.cur = 0

    def start(self, cache: "_DecodeCache") -> None:
        if not cache.prerot:
            raise NotImplementedError("the cached beam search needs the pre-rotated cache (rotary dims % 16 == 0, head size 64 / 128 / 256)")

    def before_step(self, cache: "_DecodeCache") -> None:
        cache.anc = self.anc[self.cur]

    def __call__(self, logits: torch.Tensor, t: int) -> torch.Tensor:
        B, k, cur, o = self.B, self.rows, self.cur, 1 - self.cur
        score = self.run_score
        if t == 0 and logits.shape[0] == B:   # the cached loop's prefill, one row per sample: only beam 0 is live there
            score = torch.zeros(B, dtype=torch.float32, device=self.dev)
        elif t == 0:   # the recompute loop's B * k rows (HF expands every sample k times): beams 1 .. k-1 start at -1e9, so the first
            score = torch.full((B, k), -1e9, dtype=torch.float32, device=self.dev)   # step's candidates all come from beam 0
            score[:, 0] = 0.0
            score = score.view(B * k)
        ops.beam_candidates(logits, score, B, k, out=self.cand)
        if self.trace is not None:   # tests / tools: every step's candidate lists (score, token, parent), copied
            self.trace.append(tuple(c.clone() for c in self.cand))
        cap, eos, pad, early, length_penalty = self.args
        ops.beam_update(self.cand, B, k, t, cap, eos, pad, early, length_penalty, self.run_score, (self.anc[cur], self.anc[o]),
                        (self.hist[cur], self.hist[o]), (self.fin_tok[cur], self.fin_tok[o]), (self.fin_score[cur], self.fin_score[o]),
                        (self.fin_len[cur], self.fin_len[o]), self.done, self.next_tok)
        self.cur = o
        return self.next_tok

    def drawn(self, t: int) -> torch.Tensor:
        return self.hist[self.cur][:, :t]   # re-read every step: the beams reorder

    def result(self, ids: torch.Tensor):
        B, nrs, cur = self.B, self.nrs, self.cur
        n_keep = int(self.fin_len[cur][:, :nrs].max())   # the one host synchronisation
        seqs = torch.cat([ids.repeat_interleave(nrs, 0), self.fin_tok[cur][:, :nrs, :n_keep].reshape(B * nrs, n_keep)], dim=1)
        if self.return_dict:
            return BeamSearchOutput(sequences=seqs, sequences_scores=self.fin_score[cur][:, :nrs].reshape(B * nrs).clone())
        return seqs


class GenerationMixin:
    """``generate`` and what it runs on, as methods of the model."""

    # ---- greedy decode -----------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, pixel_values: Optional[torch.Tensor] = None,
                 patch_embeddings: Optional[torch.Tensor] = None, max_new_tokens: int = 10, use_cache: bool = True,
                 pad_token_id: Optional[int] = None, eos_token_id: Optional[int] = 0, do_sample: bool = False,
                 return_step_logits: bool = False, use_graph: bool = False, num_beams: int = 1, length_penalty: float = 1.0,
                 early_stopping: Any = False, num_return_sequences: int = 1, return_dict_in_generate: bool = False,
                 image_index: Optional[torch.Tensor] = None, **kwargs):
        """Greedy search with the call signature the reference validation uses (mafed/model/vqa_cont_learner.py:260-267,
        mafed/utils/eval_utils.py:170-177: ``generate(input_ids=, attention_mask=, pixel_values=, max_new_tokens=10,
        use_cache=False, pad_token_id=eos)``) and HF ``greedy_search`` semantics (transformers 4.37.1): next token = argmax of
        the last position, finished rows keep emitting ``pad_token_id``, the attention mask grows by ones, generation stops
        when every row has produced ``eos_token_id`` (GPT-NeoX / Pythia: 0) or after ``max_new_tokens``.  Positions are
        ``arange`` over [image | text | generated].

        ``use_cache=False`` is the reference's literal behaviour -- the whole 256 + T + t prefix is pushed through the stack
        again for every token.  ``use_cache=True`` (default here) runs the prefix once, keeps each layer's fused-QKV output as
        the K/V cache and then moves ONE row per sample through the stack per token (``mafed_attn_decode``); both produce the
        same tokens.  Returns [B, T + n_generated] like HF; with ``return_step_logits`` also the fp32 last-position logits of
        every step [n, B, V].

        ``num_beams = k > 1``: beam search with HF ``GenerationMixin._beam_search`` semantics (transformers 5.x; ``length_penalty``,
        ``early_stopping`` True / False / "never", ``num_return_sequences`` <= k <= 8) -> [B * num_return_sequences, T + n], rows padded
        with ``pad_token_id`` up to the longest returned hypothesis; ``return_dict_in_generate`` adds the length-normalised
        ``sequences_scores`` (a beam-search option: the greedy path returns its tensor as before).  ``use_cache=False`` recomputes the B * k beams' full sequences every step; ``use_cache=True`` prefills
        each sample once and decodes its k beams over the shared prefix (``_BeamPick``).  Not implemented: sampling (beam-sample
        included), graph capture of the beam loop, diverse / constrained beam search.  Sampled decoding is a method of its own, ``sample``.

        ``image_index`` (int64 [B], any device): several prompts about one image.  ``patch_embeddings`` is then [N, P, Dv] (or
        ``pixel_values`` holds N images) and prompt b looks at image ``image_index[b]``; N need not equal B.  ``use_cache=False`` recomputes
        on ``feats.index_select(0, image_index)``; ``use_cache=True`` (greedy and beam) runs the image rows through the stack once per
        image and the text rows once per prompt (``_prefill_shared_rows``, DESIGN.md section 4c''').  Not with ``use_graph``."""
        if do_sample:
            raise NotImplementedError("sampling (do_sample=True, beam-sample included) is not implemented: greedy or beam search only")
        if kwargs.get("num_beam_groups") not in (None, 1) or kwargs.get("constraints") is not None or kwargs.get("force_words_ids") is not None:
            raise NotImplementedError("diverse / constrained beam search (num_beam_groups, constraints, force_words_ids) is not implemented")
        if not isinstance(num_beams, int) or num_beams < 1 or num_beams > 8:
            raise ValueError(f"num_beams must be an int in 1 .. 8, got {num_beams!r}")
        if num_return_sequences < 1 or num_return_sequences > num_beams:
            raise ValueError(f"num_return_sequences ({num_return_sequences}) must be in 1 .. num_beams ({num_beams})")
        feats, ids, am, pad_token_id = self._generate_inputs("generate", input_ids, attention_mask, pixel_values, patch_embeddings, pad_token_id, eos_token_id)
        if use_graph and image_index is not None:
            raise NotImplementedError("use_graph=True (hipGraph capture) is not implemented with image_index")
        if num_beams > 1:
            if use_graph:
                raise NotImplementedError("use_graph=True (hipGraph capture) is not implemented for beam search")
            if return_step_logits:
                raise NotImplementedError("return_step_logits is a greedy-search option")
            if max_new_tokens < 1:
                raise ValueError(f"beam search needs max_new_tokens >= 1, got {max_new_tokens}")
            if early_stopping not in (False, True, "never"):
                raise ValueError(f"early_stopping must be True, False or 'never', got {early_stopping!r}")
        feats, image_index = self._pair_images(feats, image_index, ids.shape[0], use_cache)
        if num_beams > 1:
            pick = _BeamPick(ids.shape[0], ids.device, eos_token_id, pad_token_id, num_beams, max_new_tokens, float(length_penalty), early_stopping,
                             num_return_sequences, return_dict_in_generate, self.beam_trace)
            return self._decode(pick, feats, ids, am, max_new_tokens, use_cache, image_index=image_index)
        pick = _GreedyPick(ids.shape[0], ids.device, eos_token_id, pad_token_id, return_step_logits)
        out, steps, _ = self._decode(pick, feats, ids, am, max_new_tokens, use_cache, use_graph, image_index)
        return (out, steps) if return_step_logits else out

    def _decode(self, pick, feats, ids, am, max_new: int, use_cache: bool, use_graph: bool = False, image_index: Optional[torch.Tensor] = None):
        """The decode loop of ``generate`` and ``sample`` around a pick object (``_GreedyPick``) -> ``pick.result``.  It issues launches
        only: no host synchronisation before the one in ``pick.result``."""
        B, T = ids.shape
        if not use_cache:
            # the reference's literal recompute: the B * rows full sequences through the stack for every token
            feats_r, ids_r, am_r = _rows(feats, pick.rows), _rows(ids, pick.rows), _rows(am, pick.rows)
            cur_ids, cur_am = ids_r, am_r
            for t in range(max_new):
                st = self._engine_forward(feats_r, cur_ids, cur_am, None, False, train=False)
                pick(st["logits"][:, -1, :], t)
                gen = pick.drawn(t + 1)
                cur_ids, cur_am = torch.cat([ids_r, gen], dim=1), torch.cat([am_r, torch.ones_like(gen)], dim=1)
        elif use_graph and not pick.want_steps and max_new > 1:
            # opt-in: the nine one-row-per-sample steps (~150 launches of 5-20 us kernels each) captured once per (B, T, max_new)
            # into a hipGraph whose K/V cache lives at fixed addresses (the prefill's QKV GEMMs write straight into it).  It
            # takes the host out of the loop; on an idle host it measures the same as eager launches (24.1 vs 24.2 ms at
            # 410M / B = 32): the steps are bound by the GPU-side cost of that many small kernels.
            key = (B, T, max_new, pick.eos, pick.pad) + pick.key
            gd = self._decode_graphs.get(key)
            if gd is None:
                gd = self._decode_graphs[key] = _GraphedDecode(self, B, T, max_new, pick)
            return gd.run(feats, ids, am, pick)
        else:
            # one prefill per prompt: its last-position logits are the first step's, its K/V the prefix that the prompt's rows share
            cache, first_logits = self._prefill(feats, ids, am, max_new, beams=pick.rows, image_index=image_index)
            pick.start(cache)
            self._decode_steps(pick, cache, first_logits, max_new)
        return pick.result(ids)

    def _decode_steps(self, pick, cache: "_DecodeCache", first_logits: torch.Tensor, max_new: int) -> None:
        """The cached loop: a pick from the prompt's logits, then max_new - 1 times one row per sequence through the stack and a pick
        from its logits.  Run eagerly by ``_decode`` and captured by ``_GraphedDecode``."""
        nxt = pick(first_logits, 0)
        for t in range(max_new - 1):
            pick.before_step(cache)
            nxt = pick(self._engine_decode_step(nxt, t, cache), t + 1)

    # ---- sampled decode (DESIGN.md section 4c'') -----------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, pixel_values: Optional[torch.Tensor] = None,
               patch_embeddings: Optional[torch.Tensor] = None, max_new_tokens: int = 10, use_cache: bool = True,
               pad_token_id: Optional[int] = None, eos_token_id: Optional[int] = 0, temperature: float = 1.0, top_k: int = 0,
               top_p: float = 1.0, min_p: float = 0.0, num_return_sequences: int = 1, seed: int = 0, use_graph: bool = False,
               return_step_logits: bool = False, return_logprobs: bool = False, image_index: Optional[torch.Tensor] = None):
        """Multinomial sampling with HF ``GenerationMixin.sample`` semantics (temperature, then top-k, top-p and min-p warping, one draw
        per row and step; finished rows emit ``pad_token_id``), every pick one launch of ``ops.sample_token`` (csrc/sample.hip) and
        deterministic under ``seed``: the uniform number of row r at step t is Philox4x32-10 of (seed, r, t), whichever path runs.

        -> [B * n, T + n_generated] with n = ``num_return_sequences`` (1 .. 8): row b * n + j is sample j of prompt b (HF's
        ``expand_inputs_for_generation`` order), cut like the greedy output at the slowest row's first eos.  ``return_step_logits`` adds
        the fp32 last-position logits of every step [n_generated, B * n, V], ``return_logprobs`` the drawn tokens' log-probabilities under
        the warped distribution [B * n, n_generated] (0 where a finished row emitted pad); both follow the sequences in that order.

        ``use_cache=False`` repeats the inputs n times and recomputes the whole sequence per token.  ``use_cache=True`` with n = 1 is the
        greedy cached loop with the pick replaced (``use_graph=True``: the steps replayed from one hipGraph that reads the seed from a
        device word, so a new seed needs no new capture); with n > 1 every prompt is prefilled ONCE and its n samples decode over the
        shared prefix (``ops.attn_decode_beam`` under an identity ancestry table), step 0 drawing all n tokens from the prompt's one
        logits row.  No host synchronisation inside the loop.

        ``image_index`` (int64 [B]): as in ``generate`` -- N images for B prompts, the image rows prefilled once per image (one host read of
        the index's range before the loop)."""
        n = num_return_sequences
        if not temperature > 0.0:
            raise ValueError(f"temperature must be > 0, got {temperature!r}")
        if not isinstance(top_k, int) or top_k < 0:
            raise ValueError(f"top_k must be an int >= 0 (0 = off), got {top_k!r}")
        if not 0.0 < top_p <= 1.0:
            raise ValueError(f"top_p must be in (0, 1], got {top_p!r}")
        if not 0.0 <= min_p < 1.0:
            raise ValueError(f"min_p must be in [0, 1), got {min_p!r}")
        if not isinstance(n, int) or n < 1 or n > 8:
            raise ValueError(f"num_return_sequences must be an int in 1 .. 8, got {n!r}")
        if not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"seed must be an int that fits a uint64, got {seed!r}")
        if max_new_tokens < 1:
            raise ValueError(f"sample needs max_new_tokens >= 1, got {max_new_tokens}")
        feats, ids, am, pad_token_id = self._generate_inputs("sample", input_ids, attention_mask, pixel_values, patch_embeddings, pad_token_id, eos_token_id)
        if use_graph and (n > 1 or not use_cache or return_step_logits):
            raise NotImplementedError("use_graph=True serves the cached n = 1 path without return_step_logits")
        if use_graph and image_index is not None:
            raise NotImplementedError("use_graph=True (hipGraph capture) is not implemented with image_index")
        feats, image_index = self._pair_images(feats, image_index, ids.shape[0], use_cache)
        # (a captured pick serves later calls with and without log-probabilities: it always takes them)
        pick = _SampledPick(ids.shape[0] * n, ids.device, eos_token_id, pad_token_id, (float(temperature), int(top_k), float(top_p), float(min_p)),
                            n, seed, return_step_logits, return_logprobs or use_graph)
        out = self._decode(pick, feats, ids, am, max_new_tokens, use_cache, use_graph, image_index)
        out = tuple(o for o, wanted in zip(out, (True, return_step_logits, return_logprobs)) if wanted)
        return out[0] if len(out) == 1 else out

    # ---- candidate scoring (DESIGN.md section 4c'''') -------------------------------------------------------------------
    @torch.no_grad()
    def score(self, input_ids: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, pixel_values: Optional[torch.Tensor] = None,
              patch_embeddings: Optional[torch.Tensor] = None, candidate_ids: Optional[torch.Tensor] = None,
              candidate_mask: Optional[torch.Tensor] = None, normalize: str = "sum", use_cache: bool = True,
              image_index: Optional[torch.Tensor] = None, return_token_logprobs: bool = False):
        """Log-likelihood of given answers: ``candidate_ids`` int64 [B, C, A] holds C candidate continuations of A tokens for each of the B
        prompts, ``candidate_mask`` int64 [B, C, A] their RIGHT-padded lengths (ones then zeros; None = all ones).

            score[b, c] = sum_j mask[b, c, j] * log p(cand[b, c, j] | image b, prompt b, cand[b, c, :j])

        -> fp32 [B, C]; ``normalize="mean"`` divides by the candidate's token count; a candidate without a token scores -inf, so it loses
        every ranking.  ``return_token_logprobs`` adds the fp32 [B, C, A] terms of the sum (0 at masked positions).  Token 0 is scored
        from the prompt's last position, token j >= 1 from candidate row j - 1.

        For a sample whose text is [question | answer] with the answer labelled, ``-score(normalize="mean")`` of (question, answer) is the
        reference's per-sample masked-mean cross-entropy, and its batch mean is ``compute_loss`` (mafed/model/vl_pythia.py:64-96) =
        ``model(**batch).loss`` -- without a training forward, and per sample (the forgetting signal of a replay memory).

        ``use_cache=False`` is the literal computation: the B * C sequences [image | prompt | candidate] through the engine forward, the
        image rows and the prompt C times over.  ``use_cache=True`` (default) prefills each prompt ONCE (``image_index``: each image once,
        ``_prefill_shared_rows``), keeps every layer's fused-QKV rows as the prefix, and moves only the B * C * A candidate rows through the
        stack; they attend [prefix of their prompt | own earlier tokens] through ``ops.attn_cand_fwd``.  A is right-padded internally to
        ``padded_candidate_len`` (exact: padded rows come last in their candidate and no other candidate sees them), and the last row of
        a candidate, which predicts nothing, skips the final LayerNorm and the head.  Log-probabilities are ``ops.token_logprob``, sums
        ``ops.score_reduce``.  One host read checks the mask and the token range (one more for ``image_index``); none after that.
        ``model.prefill_trace`` (a list) receives {"prefix_rows", "candidate_rows"}: the rows that went through the stack."""
        if normalize not in ("sum", "mean"):
            raise ValueError(f"normalize must be 'sum' or 'mean', got {normalize!r}")
        feats, ids, am, _ = self._generate_inputs("score", input_ids, attention_mask, pixel_values, patch_embeddings, None, None)
        cfg, dev = self.config, ids.device
        B, T = ids.shape
        cand = candidate_ids
        if not isinstance(cand, torch.Tensor) or cand.dtype != torch.int64 or cand.dim() != 3 or cand.shape[0] != B or cand.shape[1] < 1 or cand.shape[2] < 1:
            got = (tuple(cand.shape), cand.dtype) if isinstance(cand, torch.Tensor) else type(cand).__name__
            raise ValueError(f"candidate_ids must be an int64 tensor of shape [{B}, C >= 1, A >= 1], got {got}")
        if T < 1:
            raise ValueError("score needs at least one prompt position (token 0 is scored from the prompt's last position)")
        _, C, A = cand.shape
        cand = cand.to(dev).contiguous()
        mask = candidate_mask
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype != torch.int64 or tuple(mask.shape) != (B, C, A):
                got = (tuple(mask.shape), mask.dtype) if isinstance(mask, torch.Tensor) else type(mask).__name__
                raise ValueError(f"candidate_mask must be an int64 tensor of shape [{B}, {C}, {A}], got {got}")
            mask = mask.to(dev).contiguous()
            keep = mask != 0
            tok, tgt = cand * keep, torch.where(keep, cand, -1)   # embedding ids (masked: any valid id) and targets (masked: < 0 -> 0)
            not_right_padded = ((mask != 0) & (mask != 1)).any() | (mask[..., 1:] > mask[..., :-1]).any()
        else:
            tok = tgt = cand
            not_right_padded = torch.zeros((), dtype=torch.bool, device=dev)
        bad = torch.stack([not_right_padded, ((tok < 0) | (tok >= cfg.vocab_size)).any()]).tolist()   # the one host read
        if bad[0]:
            raise ValueError("candidate_mask must be right-padded: ones, then zeros, along the last dimension")
        if bad[1]:
            raise ValueError(f"candidate_ids must lie in [0, {cfg.vocab_size}) wherever candidate_mask is set")
        feats, image_index = self._pair_images(feats, image_index, B, use_cache)
        BC, V = B * C, cfg.vocab_size
        if not use_cache:
            ids_x = torch.cat([ids.repeat_interleave(C, 0), tok.view(BC, A)], dim=1)
            am_x = torch.cat([am.repeat_interleave(C, 0), torch.ones((BC, A), dtype=torch.int64, device=dev)], dim=1)
            st = self._engine_forward(feats.repeat_interleave(C, 0), ids_x, am_x, None, False, train=False)
            # text row T - 1 + j of sequence (b, c) predicts candidate token j
            rows = torch.arange(BC, device=dev)[:, None] * (T + A) + (T - 1) + torch.arange(A, device=dev)[None, :]
            tlp = ops.token_logprob(st["logits"].view(BC * (T + A), V), tgt, rows.to(torch.int32).contiguous())
        else:
            tlp, trace = self._score_shared(feats, image_index, ids, am, tok, tgt)
            if self.prefill_trace is not None:
                self.prefill_trace.append(trace)
        scores = ops.score_reduce(tlp, mask, normalize == "mean")
        return (scores, tlp) if return_token_logprobs else scores

    def _score_shared(self, feats, image_index, ids, am, tok, tgt) -> Tuple[torch.Tensor, dict]:
        """``score``'s shared path -> (token log-probabilities fp32 [B, C, A], the trace record)."""
        cfg = self.config
        P, h, H, D, L = cfg.num_vision_tokens, cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim, cfg.num_hidden_layers
        (B, T), (_, C, A), dev = ids.shape, tok.shape, ids.device
        S0, BC, rot = P + T, B * C, cfg.rotary_ndims
        store, first, _ = self._prefix_rows(feats, ids, am, image_index)
        prefix_rows = feats.shape[0] * P + B * T   # every image once (without an index: one per prompt), every prompt's text once
        # token 0 of all C candidates of a prompt reads the prompt's one logits row
        row0 = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(C)
        lp0 = ops.token_logprob(first, tgt[:, :, 0].contiguous(), row0)
        if A == 1:   # nothing to condition on: no candidate row enters the stack
            return lp0.view(B, C, 1), {"prefix_rows": prefix_rows, "candidate_rows": 0}
        A_run = self.padded_candidate_len(BC, A)
        if A_run != A:
            tok = torch.cat([tok, torch.zeros((B, C, A_run - A), dtype=torch.int64, device=dev)], dim=2)
        cos, sin = self.rotary_tables(S0 + A_run)
        wts, pars = self._tensors(0), self._tensors(1)
        x = pars.outer.embed_in.index_select(0, tok.reshape(-1))   # fp32 residual rows [B*C*A_run, h]
        for i in range(L):
            x = self._layer_forward(wts, pars, i, x, lambda qkv: (ops.attn_cand_fwd(store[i], S0, qkv, C, A_run, B, H, D, rot, cos, sin, am), None))
        # candidate row j predicts token j + 1: rows 0 .. A - 2 of every candidate go through the final LayerNorm and the head
        lp1 = ops.token_logprob(self._lm_head(x.view(BC, A_run, h)[:, :A - 1, :].reshape(BC * (A - 1), h)), tgt[:, :, 1:].contiguous())
        return torch.cat([lp0.view(B, C, 1), lp1], dim=2), {"prefix_rows": prefix_rows, "candidate_rows": BC * A_run}

    def _generate_inputs(self, what: str, input_ids, attention_mask, pixel_values, patch_embeddings, pad_token_id, eos_token_id):
        """The inputs of entry point ``what`` -> (vision features, token ids, attention mask) on the model's device and the effective
        ``pad_token_id``."""
        if input_ids is None or (pixel_values is None and patch_embeddings is None):
            raise ValueError(f"{what} needs input_ids and pixel_values / patch_embeddings")
        dev = self.flat_params.device
        feats = (patch_embeddings if patch_embeddings is not None else self.get_patch_embeddings(pixel_values)).to(dev).contiguous()
        ids = input_ids.to(dev, torch.int64).contiguous()
        am = (attention_mask if attention_mask is not None else torch.ones_like(input_ids)).to(dev, torch.int64).contiguous()
        if eos_token_id is not None and pad_token_id is None:
            pad_token_id = eos_token_id  # HF's fallback for open-end generation
        return feats, ids, am, pad_token_id

    def _prefix_store(self, B: int, T: int) -> torch.Tensor:
        """[L, B*S0, 3h]: every layer's fused-QKV output lands in one tensor (the K/V cache's prefix): its keys are then rotated by ONE launch."""
        cfg = self.config
        S0 = cfg.num_vision_tokens + T
        return torch.empty((cfg.num_hidden_layers, B * S0, 3 * cfg.num_attention_heads * cfg.head_dim), dtype=self.compute_dtype,
                           device=self.flat_params.device)

    def _pair_images(self, feats, image_index, B: int, use_cache: bool):
        """Check ``image_index`` against the N feature rows and the B prompts -> (features, index on the device or None).  Without an index
        the features must be one per prompt.  With one and ``use_cache=False`` the features come back expanded (the reference's literal
        recompute on ``feats.index_select(0, image_index)``) and the index is dropped.  One host read: the index's min and max."""
        N = feats.shape[0]
        if image_index is None:
            if N != B:
                raise ValueError(f"{N} images for {B} prompts: pass image_index (int64 [B]) to pair them")
            return feats, None
        if not isinstance(image_index, torch.Tensor) or image_index.dtype != torch.int64 or tuple(image_index.shape) != (B,):
            got = (tuple(image_index.shape), image_index.dtype) if isinstance(image_index, torch.Tensor) else type(image_index).__name__
            raise ValueError(f"image_index must be an int64 tensor of shape [{B}], got {got}")
        idx = image_index.to(feats.device).contiguous()
        lo, hi = torch.stack(idx.aminmax()).tolist() if B else (0, -1)
        if lo < 0 or hi >= N:
            raise ValueError(f"image_index values must lie in [0, {N}), got {lo} .. {hi}")
        if not use_cache:
            return feats.index_select(0, idx), None
        return feats, idx

    def _prefill(self, feats, ids, am, cap: int, beams: int = 1, image_index: Optional[torch.Tensor] = None) -> Tuple["_DecodeCache", torch.Tensor]:
        """Run the prompt once, its QKV GEMMs writing straight into a fresh prefix store -> (the decode cache over it, the last
        position's logits [B, V]).  With ``image_index``: over the shared-image prefix of ``_prefix_rows`` (DESIGN.md section 4c''')."""
        store, logits, record = self._prefix_rows(feats, ids, am, image_index)
        if record is not None and self.prefill_trace is not None:   # tests / tools: the row counts that went through the stack
            self.prefill_trace.append(record)
        B, T = ids.shape
        cache = _DecodeCache(self, list(store.unbind(0)), B, self.config.num_vision_tokens + T, cap, am, fused=self.fused_decode,
                             prefix_storage=store, beams=beams)   # (rotates the prefix keys)
        return cache, logits

    def _prefix_rows(self, feats, ids, am, image_index: Optional[torch.Tensor] = None, store: Optional[torch.Tensor] = None):
        """The prefix rows of a prompt -> (prefix store [L, B*S0, 3h] with un-rotated keys, the last position's logits [B, V], the trace
        record or None).  Without ``image_index`` the engine forward's QKV GEMMs write straight into a fresh store (or the given ``store``,
        the captured graph's) and there is no record; with it the image rows run once per image: ``_prefill_shared_rows``."""
        if image_index is not None:
            return self._prefill_shared_rows(feats, image_index, ids, am)
        store = self._prefix_store(*ids.shape) if store is None else store
        st = self._engine_forward(feats, ids, am, None, False, train=False, qkv_out=list(store.unbind(0)), last_only=True)
        return store, st["logits"][:, -1, :], None

    def _prefill_shared_rows(self, feats, image_index, ids, am) -> Tuple[torch.Tensor, torch.Tensor, dict]:
        """The prompt rows of B prompts over the N images of ``feats`` -> (prefix store [L, B*S0, 3h] with un-rotated keys, the last position's
        logits [B, V], the trace record).  The prompt is [image | text], fully causal with
        arange positions, so the image rows of every layer depend on the image alone.  They go through the stack once per image (their
        fused-QKV rows into an image store [L, N*P, 3h]; the last layer stops there, nothing reads its image rows), the text rows once
        per prompt (text store [L, B*T, 3h]), attending [image image_index[b] | own text] through ``ops.attn_suffix_fwd``; one gather then
        lays the two stores out as the [L, B*S0, 3h] prefix the decode cache takes.  The layer body is the engine's ``_layer_forward``."""
        if not self.flat_params.is_cuda:
            raise RuntimeError("mafed_amd runs on the GPU only (no CPU fallback); move the model with .cuda()")
        cfg, cd = self.config, self.compute_dtype
        P, h, H, D, L = cfg.num_vision_tokens, cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim, cfg.num_hidden_layers
        # behind every chunk of a pipelined optimiser update at once, where the engine forward orders itself layer by layer
        self._params_ready(torch.cuda.current_stream(), -1, L + 1)
        (B, T), N = ids.shape, feats.shape[0]
        S0, rot, eps, dev = P + T, cfg.rotary_ndims, cfg.layer_norm_eps, ids.device
        cos, sin = self.rotary_tables(S0)
        wts, pars = self._tensors(0), self._tensors(1)
        img_store = torch.empty((L, N * P, 3 * h), dtype=cd, device=dev)
        txt_store = torch.empty((L, B * T, 3 * h), dtype=cd, device=dev)

        # image pass, N * P rows: projector, then the layers over the image alone (S = P; the one-column mask of ones makes the last image
        # key a valid "text" key of the full attention kernels, which take T >= 1 through this wrapper)
        img = self._projector_forward(feats, N, False)[3]
        x = img if img.dtype == torch.float32 else ops.cast(img, torch.float32)   # fp32 residual stream
        ones = torch.ones((N, 1), dtype=torch.int64, device=dev)
        for i in range(L):
            if i == L - 1:
                w, p = wts.layers[i], pars.layers[i]
                ln1, _, _, _ = ops.layernorm_fwd(x, p.ln1_w, p.ln1_b, None, None, eps, cd, save_stats=False)
                ops.gemm(ln1, w.qkv_w, False, True, bias=p.qkv_b, out=img_store[i])
                break
            x = self._layer_forward(wts, pars, i, x, lambda qkv: ops.attn_fwd(qkv, N, P, H, D, rot, cos, sin, ones), qkv_out=img_store[i])
        # text pass, B * T rows
        x = pars.outer.embed_in.index_select(0, ids.reshape(-1))
        for i in range(L):
            x = self._layer_forward(wts, pars, i, x, lambda qkv: (ops.attn_suffix_fwd(img_store[i], image_index, N, P, qkv, T, B, H, D, rot, cos, sin, am), None),
                                    qkv_out=txt_store[i])
        logits = self._lm_head(x.view(B, T, h)[:, -1, :].contiguous())
        # prefix assembly: [image of the prompt | its text] per layer, one launch for all of them
        store = ops.prefix_gather(img_store, txt_store, image_index, B, P, T, out=self._prefix_store(B, T))
        return store, logits, {"image_store": tuple(img_store.shape), "text_store": tuple(txt_store.shape), "prefix": tuple(store.shape)}

    def _engine_decode_step(self, tokens: torch.Tensor, t: int, cache: "_DecodeCache") -> torch.Tensor:
        """One token per sample through the stack: ``tokens`` [B] sit at position S0 + t; returns the logits [B, V]."""
        cfg = self.config
        h, H, D, L = cfg.hidden_size, cfg.num_attention_heads, cfg.head_dim, cfg.num_hidden_layers
        B, S0, rot = cache.B, cache.S0, cfg.rotary_ndims
        cos, sin = self.rotary_tables(S0 + cache.cap)
        wts, pars = self._tensors(0), self._tensors(1)   # compute-dtype weights; fp32 LayerNorm parameters, biases and embedding
        Wo, Po = wts.outer, pars.outer
        x = Po.embed_in.index_select(0, tokens)  # fp32 residual stream row

        def attend(i):
            # (greedy: one cache row per sample; beam search: `anc` names the slot holding each row of a beam's history.  A fused cache
            #  is always pre-rotated, _DecodeCache)
            if cache.anc is None:
                return ops.attn_decode(cache.prefix[i], S0, cache.new[i], t, B, H, D, rot, cos, sin, cache.attention_mask, prerot=cache.prerot)
            return ops.attn_decode_beam(cache.prefix[i], S0, cache.new[i], t, B, cache.beams, cache.anc, H, D, rot, cos, sin, cache.attention_mask)

        for i in range(L):
            w, p = wts.layers[i], pars.layers[i]
            if cache.fused:
                # three launches per layer (csrc/decode.hip): [LN1 | LN2] + QKV + fc1/GELU, attention over the pre-rotated cache, and
                # dense + fc2 + both residuals as one product over the concatenated K
                a = ops.decode_ln_qkv_fc1(x, p.ln1_w, p.ln1_b, p.ln2_w, p.ln2_b, cfg.layer_norm_eps, w.qkv_w, p.qkv_b, cache.new[i][:, t, :],
                                          w.fc1_w, p.fc1_b)
                x = ops.decode_out(x, attend(i), a, w.dense_w, p.dense_b, w.fc2_w, p.fc2_b, cache.workspace, out=x)
                continue
            # the new token's q | k | v row goes straight into the cache (row t of the per-layer [B, cap, 3*H*D] tensor)
            x = self._layer_forward(wts, pars, i, x, lambda qkv: (attend(i), None), qkv_out=cache.new[i][:, t, :])
        if cache.fused and B * cache.beams <= 32 and h == 1024 and cfg.vocab_size % 32 == 0 and cfg.vocab_size >= 16384:
            # final LayerNorm + LM head as one persistent launch (decode_head_kernel: rows normalised once per CU, the vocabulary's
            # weight strips streamed through LDS): 24 us against 48 for LayerNorm + the skinny product at V = 50k
            return ops.decode_ln_linear(x, Po.final_ln_w, Po.final_ln_b, cfg.layer_norm_eps, Wo.embed_out)
        # (other shapes: the one-slab-per-block forms of ops.decode_ln_linear are no faster than the two launches below)
        return self._lm_head(x)


class _DecodeCache:
    """K/V cache of a greedy decode: per layer the prefill's [B*S0, 3*H*D] fused-QKV output (kept as written -- no split, no
    transpose, k un-rotated) and a [B, cap, 3*H*D] tensor that receives one row per generated token."""

    def __init__(self, model, prefix, B: int, S0: int, cap: int, attention_mask: torch.Tensor, prerotate: bool = True, fused: bool = True,
                 prefix_storage: Optional[torch.Tensor] = None, beams: int = 1):
        self.prefix, self.B, self.S0, self.cap, self.attention_mask = prefix, B, S0, max(1, cap), attention_mask
        self.prefix_storage = prefix_storage   # [L, B*S0, 3h] holding every entry of `prefix` (then one rotation launch serves all layers)
        # beam search: the prefix stays one per sample, the generated rows are one per beam slot ([B*beams, cap, 3h]); `anc` (int32
        # [B*beams, cap], set by the caller before each step) names the slot holding each row of a beam's history
        self.beams, self.anc = beams, None
        rows = B * beams
        cfg = model.config
        n = 3 * cfg.num_attention_heads * cfg.head_dim
        self.new = [torch.zeros((rows, self.cap, n), dtype=prefix[0].dtype, device=prefix[0].device) for _ in prefix]
        # Pre-rotated cache (round 4): once the prefill's attention has read the un-rotated keys, rotate them in place -- every decode step
        # then loads k and v only (mafed_attn_decode_prerot).  Needs rot % 16 == 0 and an MFMA head size (every VLPythia preset).
        self.prerot = bool(prerotate) and cfg.rotary_ndims % 16 == 0 and cfg.head_dim in (64, 128, 256)
        self._model = model
        # fused decode layer (csrc/decode.hip): bf16 mode over the pre-rotated cache, shapes per mafed_decode_supported
        # (more than 64 rows -- 64-row blocks of the fused kernels -- only for beam search: a greedy batch of B > 64 keeps the six launches)
        self.fused = (bool(fused) and self.prerot and prefix[0].dtype == torch.bfloat16 and (rows <= 64 or beams > 1)
                      and ops.decode_supported(rows, cfg.hidden_size, cfg.intermediate_size))
        self.workspace = ops.decode_out_workspace(rows, cfg.hidden_size, prefix[0].device) if self.fused else None
        if self.prerot:
            self.rotate_prefix()

    def rotate_prefix(self) -> None:
        """Rotate the prefix keys in place (call once per prefill: the prefix must hold what the QKV GEMMs wrote)."""
        cfg = self._model.config
        cos, sin = self._model.rotary_tables(self.S0 + self.cap)
        whole = self.prefix_storage   # every layer's prefix in ONE tensor: one launch for all
        if whole is not None:
            ops.rotate_k_rows_(whole, whole.shape[0] * self.B, self.S0, cfg.num_attention_heads, cfg.head_dim, cfg.rotary_ndims, cos, sin)
            return
        for p in self.prefix:
            ops.rotate_k_rows_(p, self.B, self.S0, cfg.num_attention_heads, cfg.head_dim, cfg.rotary_ndims, cos, sin)


class _GraphedDecode:
    """The decode steps of ``_decode_steps`` for one (B, T, max_new) shape and one pick object as a single hipGraph.  Static buffers: the
    per-layer K/V cache (prefix written by the prefill's QKV GEMMs through ``qkv_out``, plus the per-token rows), the prompt mask, the
    prefill's last-position logits and what the pick owns: the capture leaves its tokens (and log-probabilities) at fixed addresses, which
    every replay fills again; ``pick.inputs`` (the sampled pick's seed word) are rewritten by ``run`` before the replay."""

    def __init__(self, model, B: int, T: int, max_new: int, pick):
        cfg = model.config
        dev, cd = model.flat_params.device, model.compute_dtype
        S0 = cfg.num_vision_tokens + T
        self.model, self.pick = model, pick
        store = model._prefix_store(B, T)
        self.am = torch.ones((B, T), dtype=torch.int64, device=dev)
        self.first_logits = torch.zeros((B, cfg.vocab_size), dtype=cd, device=dev)
        model.rotary_tables(S0 + max(1, max_new))  # built (host -> device copy) before the capture, not inside it
        self.cache = _DecodeCache(model, list(store.unbind(0)), B, S0, max_new, self.am, fused=model.fused_decode,
                                  prefix_storage=store)   # (rotates the still-empty prefix once: harmless)

        def body():
            pick.reset()   # inside the capture: every replay starts from fresh ``unfinished`` flags
            model._decode_steps(pick, self.cache, self.first_logits, max_new)

        # one eager pass on a side stream (lazy initialisations must not happen inside the capture), then the capture
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            body()

    def run(self, feats, ids, am, pick):
        """Prefill into the static cache, replay -> the captured pick's result; ``pick``: this call's, of the captured one's key."""
        for mine, given in zip(self.pick.inputs, pick.inputs):
            mine.copy_(given)
        _, first_logits, _ = self.model._prefix_rows(feats, ids, am, store=self.cache.prefix_storage)
        if self.cache.prerot:
            self.cache.rotate_prefix()   # this prefill's keys, rotated in place for the captured steps
        self.am.copy_(am)
        self.first_logits.copy_(first_logits)
        self.graph.replay()
        return self.pick.result(ids)
