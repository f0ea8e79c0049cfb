"""Sampler with SGLang's interface (reference:
/root/reference/python/sglang/srt/layers/sampler.py:71-300, SamplingBatchInfo in
srt/sampling/sampling_batch_info.py), running the gfx950 sampling kernels."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, List, Optional

import torch
from torch import nn

from .. import kernels

TOP_K_ALL = 1 << 30   # srt/sampling/sampling_params.py:40


@dataclass
class SamplingBatchInfo:
    temperatures: torch.Tensor            # [B, 1] fp32
    top_ps: torch.Tensor                  # [B] fp32
    top_ks: torch.Tensor                  # [B] int32 (TOP_K_ALL = whole vocab)
    min_ps: torch.Tensor                  # [B] fp32
    is_all_greedy: bool = True
    need_top_p_sampling: bool = False
    need_top_k_sampling: bool = False
    need_min_p_sampling: bool = False
    sampling_seed: Optional[torch.Tensor] = None   # [B] int64 -> deterministic gumbel sampling
    sync_token_ids_across_tp: bool = False

    def filter_batch(self, keep_indices) -> "SamplingBatchInfo":
        """The rows `keep_indices` of this batch, in that order (srt/sampling/sampling_batch_info.py filter_batch: the
        scheduler calls it when requests leave the running batch -- finished or retracted)."""
        idx = torch.as_tensor(keep_indices, dtype=torch.int64, device=self.top_ps.device)
        return SamplingBatchInfo(self.temperatures[idx], self.top_ps[idx], self.top_ks[idx], self.min_ps[idx], self.is_all_greedy,
                                 self.need_top_p_sampling, self.need_top_k_sampling, self.need_min_p_sampling,
                                 self.sampling_seed[idx] if self.sampling_seed is not None else None, self.sync_token_ids_across_tp)

    @classmethod
    def greedy(cls, batch: int, device) -> "SamplingBatchInfo":
        return cls(torch.ones((batch, 1), device=device), torch.ones(batch, device=device),
                   torch.full((batch,), TOP_K_ALL, dtype=torch.int32, device=device),
                   torch.zeros(batch, device=device), True)


@dataclass
class LogitsProcessorOutput:
    next_token_logits: torch.Tensor       # [B, vocab] fp32, or the model dtype (widened on use)
    hidden_states: Optional[torch.Tensor] = None
    # filled by the sampler when return_logprob (logits_processor.py LogitsProcessorOutput fields)
    next_token_logprobs: Optional[torch.Tensor] = None
    next_token_top_logprobs_val: Optional[List] = None
    next_token_top_logprobs_idx: Optional[List] = None
    next_token_token_ids_logprobs_val: Optional[List] = None
    next_token_token_ids_logprobs_idx: Optional[List] = None


# which route the non-greedy batches, and the return_logprob calls, of this process took (tests / telemetry: tests/golden/ref_model.py reports it)
served = {"one_call_from_logits": 0, "softmax_then_sample": 0, "logprobs_from_logits": 0, "logprobs_full_matrix": 0}


class Sampler(nn.Module):
    """sampler.py:71-300.  Dtypes follow the reference: greedy ids are int64 (torch.argmax, :139), sampled ids
    int32 (sampling_from_probs_torch / the torch top-k/top-p path).  Unseeded sampling draws one fresh 62-bit seed
    per row from torch's device generator inside kernels.top_k_top_p_min_p_sample (graph-safe philox), so
    `sampling_info.sampling_seed is None` means "non-deterministic", exactly like torch.multinomial in the
    reference's unseeded path."""

    def forward(self, logits_output: LogitsProcessorOutput, sampling_info: SamplingBatchInfo,
                return_logprob: bool = False, top_logprobs_nums: Optional[List[int]] = None,
                token_ids_logprobs: Optional[List[List[int]]] = None, positions: Optional[torch.Tensor] = None
                ) -> torch.Tensor:
        logits = logits_output.next_token_logits
        if logits.shape[0] == 0:
            return torch.empty((0,), dtype=torch.int64, device=logits.device)
        # custom logit processors + NaN handling of the reference instance this forward is bound to (sampler.py:126)
        pre = getattr(self, "_preprocess_logits", None)
        if pre is not None:
            logits = pre(logits, sampling_info)
        logprobs = None
        # return_logprob, standalone (no output_logprob_processor bound: that interface needs the full matrix): the logprob outputs
        # come from ONE pass over the logits (kernels.logprobs_from_logits), whenever the logits survive the sampling call
        from_logits = return_logprob and self._logprobs_from_logits_ok(top_logprobs_nums)
        src, src_temperatures = logits, None           # what the logprob kernel reads: the logits as handed in
        if sampling_info.is_all_greedy:
            ids = kernels.argmax(logits)                                    # sampler.py:133-141
            if return_logprob and not from_logits:
                logprobs = torch.log_softmax(logits.float(), dim=-1)        # :143-146
        else:
            # sampler.py:148-152, 211-260: div_ temperature, softmax in place, then sample from probs
            simple_sampling_case = not (sampling_info.need_top_p_sampling or sampling_info.need_top_k_sampling
                                        or sampling_info.need_min_p_sampling)
            probs = ids = None
            min_ps = sampling_info.min_ps if sampling_info.need_min_p_sampling else None
            src_temperatures = sampling_info.temperatures
            if not return_logprob or from_logits:
                # The logits of a decode-sized batch (bf16, or the fp32 the reference's LogitsProcessor hands over).  Filtered sampling:
                # ONE native call, the probabilities are never written (and the logits not overwritten with them: sampler.py:216 does
                # that in place; the logprob kernel reads the untouched logits afterwards); otherwise bf16 logits are widened inside the
                # softmax launches (exact; no separate pass)
                if not simple_sampling_case:
                    ids = kernels.sample_from_logits(logits, sampling_info.temperatures, sampling_info.top_ks, sampling_info.top_ps,
                                                     min_ps, sampling_info.sampling_seed, positions)
                    served["one_call_from_logits" if ids is not None else "softmax_then_sample"] += 1
                if ids is None and logits.dtype == torch.bfloat16:
                    probs = kernels.softmax_temperature_from_bf16(logits, sampling_info.temperatures)
            # the in-place fp32 softmax overwrites fp32 logits before the ids exist: those calls keep the log(probs) route
            from_logits = from_logits and (ids is not None or src.dtype == torch.bfloat16)
            if ids is None:
                if probs is None:
                    if logits.dtype != torch.float32:
                        logits = logits.float()                             # exact widening of the bf16 logits
                    probs = kernels.softmax_temperature_(logits, sampling_info.temperatures)
                if simple_sampling_case:
                    ids = kernels.top_k_top_p_min_p_sample(probs, None, None, None, sampling_info.sampling_seed, positions,
                                                           filtered=False)
                else:
                    ids = kernels.top_k_top_p_min_p_sample(probs, sampling_info.top_ks, sampling_info.top_ps, min_ps,
                                                           sampling_info.sampling_seed, positions)
            if return_logprob and not from_logits:
                logprobs = torch.log(probs)                                 # :252-257
        if return_logprob:
            served["logprobs_from_logits" if from_logits else "logprobs_full_matrix"] += 1
            if from_logits:
                self._write_logprobs_from_logits(logits_output, src, src_temperatures, ids, top_logprobs_nums, token_ids_logprobs)
            else:
                self._write_logprobs(logits_output, logprobs, ids, top_logprobs_nums, token_ids_logprobs)
        self._sync_token_ids_across_tp(ids, sampling_info)     # in place, like the reference's (returns None there)
        return ids

    def _logprobs_from_logits_ok(self, top_logprobs_nums) -> bool:
        """The logprob kernel serves the standalone sampler with top lists up to its compile-time cap; bound to a reference Sampler
        the instance's output_logprob_processor is handed the full matrix as before."""
        return (getattr(self, "output_logprob_processor", None) is None
                and max(top_logprobs_nums or [0]) <= kernels.logprobs_max_top())

    def _write_logprobs_from_logits(self, logits_output, logits, temperatures, ids, top_logprobs_nums, token_ids_logprobs) -> None:
        """The five logprob fields of _write_logprobs (same types and shapes) from kernels.logprobs_from_logits: no [B, V]
        log-probability matrix, no topk over it.  The one intended difference: a token whose probability underflows in fp32 gets
        its finite log-probability (z - logsumexp(z)) where log(probs) gave -inf."""
        k = max(top_logprobs_nums) if top_logprobs_nums else 0
        chosen, top_val, top_idx, req_val = kernels.logprobs_from_logits(logits, temperatures, ids, k, token_ids_logprobs)
        logits_output.next_token_logprobs = chosen
        if k > 0:
            vals, idx = top_val.tolist(), top_idx.tolist()
            logits_output.next_token_top_logprobs_val = [v[:n] for v, n in zip(vals, top_logprobs_nums)]
            logits_output.next_token_top_logprobs_idx = [i[:n] for i, n in zip(idx, top_logprobs_nums)]
        if token_ids_logprobs and any(t is not None for t in token_ids_logprobs):
            flat, at, out = req_val.tolist(), 0, []
            for t in token_ids_logprobs:
                n = len(t) if t is not None else 0
                out.append(flat[at:at + n])
                at += n
            logits_output.next_token_token_ids_logprobs_val = out
            logits_output.next_token_token_ids_logprobs_idx = [list(t) if t is not None else [] for t in token_ids_logprobs]

    def _write_logprobs(self, logits_output, logprobs, ids, top_logprobs_nums, token_ids_logprobs) -> None:
        """sampler.py:262-271: bound to a reference Sampler the instance's own output_logprob_processor does it;
        standalone, the same three outputs are produced with plain torch indexing (off the hot path)."""
        proc = getattr(self, "output_logprob_processor", None)
        if proc is not None:
            proc.compute_logprobs(logprobs, top_logprobs_nums, token_ids_logprobs, ids).write_output_to(logits_output)
            return
        rows = torch.arange(ids.shape[0], device=ids.device)
        logits_output.next_token_logprobs = logprobs[rows, ids.long()]
        if top_logprobs_nums and any(n > 0 for n in top_logprobs_nums):
            k = max(top_logprobs_nums)
            vals, idx = logprobs.topk(k, dim=-1)
            logits_output.next_token_top_logprobs_val = [v[:n].tolist() for v, n in zip(vals, top_logprobs_nums)]
            logits_output.next_token_top_logprobs_idx = [i[:n].tolist() for i, n in zip(idx, top_logprobs_nums)]
        if token_ids_logprobs and any(t is not None for t in token_ids_logprobs):
            logits_output.next_token_token_ids_logprobs_val = [
                logprobs[b, torch.tensor(t, device=logprobs.device)].tolist() if t is not None else []
                for b, t in enumerate(token_ids_logprobs)]
            logits_output.next_token_token_ids_logprobs_idx = [list(t) if t is not None else [] for t in token_ids_logprobs]

    def _sync_token_ids_across_tp(self, ids: torch.Tensor, sampling_info: SamplingBatchInfo) -> None:
        """sampler.py:497-512: MIN all-reduce of the ids (greedy and sampled alike) when requested (grammar / env)."""
        from ..distributed import parallel_state as ps

        if (getattr(sampling_info, "sync_token_ids_across_tp", False) and ps.get_tensor_model_parallel_world_size() > 1
                and ps.get_tp_group() is not None):
            import torch.distributed as dist

            dist.all_reduce(ids, op=dist.ReduceOp.MIN, group=ps.get_tp_group())


def accept_verified_tree(logits_output, sampling_info: Optional[SamplingBatchInfo], candidates: torch.Tensor, next_token: torch.Tensor,
                         next_sibling: torch.Tensor, uniform: Optional[torch.Tensor] = None, uniform_final: Optional[torch.Tensor] = None,
                         threshold_single: float = 1.0, threshold_acc: float = 1.0):
    """The accept step of a TARGET_VERIFY forward (eagle_info.py EagleVerifyInput.verify without the [B * nd, V] softmax):
    `logits_output` = the forward's LogitsProcessorOutput (or its next_token_logits [B * nd, V]), `sampling_info` the batch's
    (None or all-greedy: verify_tree_greedy), the tree tables from kernels.build_verify_tree.
    Returns kernels.tree_accept_from_logits' (accept_index, accept_len, bonus_token, last_node)."""
    logits = getattr(logits_output, "next_token_logits", logits_output)
    temperatures = None
    if sampling_info is not None and not sampling_info.is_all_greedy:
        asked = [n for n, on in (("top-k", sampling_info.need_top_k_sampling), ("top-p", sampling_info.need_top_p_sampling),
                                 ("min-p", sampling_info.need_min_p_sampling)) if on]
        if asked:
            raise NotImplementedError(f"accept_verified_tree: the fused tree-accept path samples from softmax(logits / T) only; "
                                      f"this batch asks for {', '.join(asked)} filtering, which it does not apply")
        temperatures = sampling_info.temperatures
    return kernels.tree_accept_from_logits(logits, temperatures, candidates, next_token, next_sibling, uniform, uniform_final,
                                           threshold_single, threshold_acc)


_SAMPLER_BACKENDS = {"hip": lambda: Sampler()}


def register_sampler_backend(name: str, factory) -> None:
    """sampler.py:531-542."""
    _SAMPLER_BACKENDS[name] = factory


def create_sampler(backend: str = "hip") -> Sampler:
    if backend not in _SAMPLER_BACKENDS:
        raise ValueError(f"Unknown sampling backend '{backend}'. Register it via register_sampler_backend().")
    return _SAMPLER_BACKENDS[backend]()
