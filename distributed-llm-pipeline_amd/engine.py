"""Python front-end of the native pipeline engine (csrc/runtime/engine.cpp).

    eng = Engine(gguf="model.gguf", stages=2, n_mb=2, mb_size=4, max_ctx=2048)
    out, stats = eng.generate([[1, 15, 27], [1, 99]], n_predict=32)

Config keys mirror the C++ Engine (see engine.h): gguf | synthetic+ftype, mode ("local" or "mp"),
stages, devices, link ("local" | "rccl" | "tcp"), backend ("hip" | "cpu"), gpu_layers (llama-cli -ngl N:
0 < N < n_layer puts the first n_layer - N layers on a CPU stage in front of the GPU stages), n_mb, mb_size, max_ctx,
prefill_chunk, split ("even" | "mem" | "cost"), graphs, fused_attn, prefill_gemm, attn_split_len,
temp/top_k/top_p/min_p/seed (sampling; llama.cpp chain order), repeat_penalty/repeat_last_n/
frequency_penalty/presence_penalty (penalties over the last n tokens, prompt included), world/rank/hosts/next_host/base_port/rccl_ids (mp mode),
threads (CPU backend), trace, watchdog_s, link_timeout_s, fault (fault injection), verbose, log_file,
kv_dtype ("f16" | "fp8"), v_blocked (HIP V pages [8][Dp][8] per kv head instead of V^T [Dp][64]; default true; saved
state is the same either way), kv_pool_tokens (paged KV pool), prefill_gemm_v (0 auto | 1 | 2 | 3 | 4), prefill_flash,
deterministic, fused_norm, small_gemv, act_dtype (stage-boundary wire: "auto" | "f32" | "bf16" | "f16"),
device_speed ("probe" or a list; Halda-style partition weights), n_probs (token logprobs: 0 off, -1 the
chosen token's only, 1..20 plus that many alternatives; read with logprobs()), row_sampling (per-request
sampling: every sequence slot has its own record, see set_slot_sampling), row_masks (a token mask per
sequence slot for constrained output, see set_slot_masks and mipipe.grammar; switches row_sampling on),
lora_adapters (LoRA adapter capacity, 0 off, at most 8; see load_adapter / set_slot_adapters) and
lora_max_rank (largest rank of an adapter tensor pair, default 64, at most 128), context_shift (default
False: a sequence that fills max_ctx ends; True: decode() / generate() first drop half of what follows the
first n_keep prompt tokens, in whole 64-token pages, and go on, see context_shift) and n_keep (default 0;
-1: the whole prompt).
"""
from __future__ import annotations

import ctypes
import json

import numpy as np

from . import _native as N


class Engine:
    def __init__(self, **cfg):
        self.cfg = dict(cfg)
        L = N.lib()
        h = L.mp_engine_create(N.cstr(json.dumps(self.cfg)))
        if not h:
            N.check(None, "engine create")
        self._h = ctypes.c_void_p(h)
        self.info = N.jcall(L.mp_engine_info, self._h, what="engine info")
        self.n_seq_cap = self.info["n_mb"] * self.info["mb_size"]

    def close(self):
        if getattr(self, "_h", None):
            N.lib().mp_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @staticmethod
    def _flat(prompts):
        lens = np.asarray([len(p) for p in prompts], np.int32)
        flat = np.asarray([t for p in prompts for t in p], np.int32)
        return flat, lens

    def generate(self, prompts, n_predict: int):
        flat, lens = self._flat(prompts)
        out = np.full((len(prompts), n_predict), -1, np.int32)
        self._n_seq = len(prompts)
        stats = N.jcall(N.lib().mp_engine_generate, self._h, flat.ctypes.data, lens.ctypes.data, len(prompts),
                        n_predict, out.ctypes.data, what="generate")
        return out.tolist(), stats

    def spec_generate(self, prompts, n_predict: int, draft_max: int = 4, ngram: int = 3):
        """Greedy speculative decoding by prompt lookup (drafts from each sequence's own context,
        one verify chunk per micro-batch per round); output equals generate() at temp 0."""
        flat, lens = self._flat(prompts)
        out = np.full((len(prompts), n_predict), -1, np.int32)
        stats = N.jcall(N.lib().mp_engine_spec_generate, self._h, flat.ctypes.data, lens.ctypes.data, len(prompts),
                        n_predict, draft_max, ngram, out.ctypes.data, what="spec_generate")
        return out.tolist(), stats

    def set_slot_sampling(self, slot: int, _for_start: bool = False, **fields):
        """Per-request sampling (Engine(row_sampling=True)): the record the next start() / admit() of the
        idle slot `slot` uses.  Fields: temp, top_k, top_p, min_p, repeat, freq, presence (absent = the
        engine's values; temp <= 0 = greedy), seed (the request's own random stream; absent = a default
        one, reported by slot_sampling), draw0 (draws already consumed: the request continues its
        stream there), logit_bias ([[id, bias], ..], bias False or -inf bans the token; at most 32).
        The d-th token a request generates is drawn with u = (mix64(seed ^ mix64(d << 20)) >> 40) / 2^24
        whatever slot, micro-batch or round it runs in.  release() puts the slot back to the defaults."""
        f = dict(fields)
        for k, v in f.items():   # JSON carries no NaN / inf: refuse them here, by name, as the engine would
            if isinstance(v, float) and not np.isfinite(v):
                raise RuntimeError(f"set_slot_sampling: bad value for {k}")
        if f.get("seed") is not None:
            f["seed"] = str(int(f["seed"]))
        if f.get("logit_bias") is not None:
            lb = f["logit_bias"]
            lb = list(lb.items()) if isinstance(lb, dict) else list(lb)
            f["logit_bias"] = [[int(i), False if (b is False or b == float("-inf")) else float(b)] for i, b in lb]
        N.check(N.lib().mp_engine_set_slot_sampling(self._h, int(slot), N.cstr(json.dumps(f)), int(_for_start)),
                "set_slot_sampling")

    def slot_sampling(self, slot: int) -> dict:
        """The record of a slot, with the seed in use (int)."""
        j = N.jcall(N.lib().mp_engine_slot_sampling, self._h, int(slot), what="slot_sampling")
        j["seed"] = int(j["seed"])
        return j

    @property
    def row_masks(self) -> bool:
        """Whether the engine was built with row_masks (set_slot_masks raises without it)."""
        return bool(N.lib().mp_engine_row_masks(self._h))

    def set_slot_masks(self, slots, masks, _for_start: bool = False):
        """Per-slot token masks (Engine(row_masks=True)): masks[i] is a uint32 array of
        ceil(vocab / 32) words for slot slots[i] (token t allowed iff masks[i][t >> 5] >> (t & 31) & 1,
        what mipipe.grammar's State.mask() returns) or None to clear the slot's mask.  From the slot's
        next token on every other token is banned, after the logit bias and the penalties and before
        the cuts and the draw.  Legal for idle slots before admit() and between decode() calls for running
        slots.  The masks of a generation's FIRST tokens go through start(..., masks=) / admit(..., masks=):
        start() clears every mask the generation before it left, so a mask set here for a slot that is
        still busy with that generation (it was never released) would not survive it; those arguments
        mark the masks as meant for the call.  release() clears a slot's mask, load_state() all of them."""
        slots = [int(s) for s in slots]
        if len(slots) != len(masks):
            raise ValueError("set_slot_masks: one mask or None per slot")
        nw = (self.info["model"]["vocab"] + 31) // 32
        keep = []
        ptrs = (ctypes.c_void_p * max(len(slots), 1))()
        for i, m in enumerate(masks):
            if m is None:
                ptrs[i] = None
                continue
            a = np.ascontiguousarray(m, dtype=np.uint32)
            if a.size != nw:
                raise ValueError(f"set_slot_masks: a mask has {a.size} words, {nw} expected")
            keep.append(a)
            ptrs[i] = a.ctypes.data
        sl = np.asarray(slots, np.int32)
        N.check(N.lib().mp_engine_set_slot_masks(self._h, sl.ctypes.data, len(slots), ptrs, int(_for_start)),
                "set_slot_masks")

    def load_adapter(self, path: str) -> int:
        """Load a llama.cpp LoRA adapter GGUF (Engine(lora_adapters=n)); returns its id, the lowest free
        one.  Every stage takes the tensor pairs of its own layers.  Raises when all ids are in use or
        the file is refused (wrong type / architecture, a tensor the engine takes no adapter on, a
        shape or rank that does not fit), naming the tensor or field."""
        return N.check(N.lib().mp_engine_load_adapter(self._h, N.cstr(str(path))), "load_adapter")

    def unload_adapter(self, adapter_id: int):
        """Free an adapter id; refused while a slot is bound to it."""
        N.check(N.lib().mp_engine_unload_adapter(self._h, int(adapter_id)), "unload_adapter")

    def adapters(self) -> list:
        """The loaded adapters: [{"id", "path", "alpha", "rank_min", "rank_max", "bytes"}]."""
        return N.jcall(N.lib().mp_engine_adapters, self._h, what="adapters")

    def set_slot_adapters(self, slots, ids, scales=None, _for_start: bool = False):
        """Bind sequence slot slots[i] to adapter ids[i] (-1 or None: the base model) at user scale
        scales[i] (default 1): the slot's rows get scale * alpha / r * B (A x) added to the projections
        the adapter covers, from its next prefill chunk or decode step on.  One adapter per slot.  Legal
        for idle slots before admit() and between decode() calls for running slots; no graph is
        re-captured.  Bindings of a generation's prompts go through start(..., adapters=) /
        admit(..., adapters=).  release() clears a slot's binding, start() those of the generation
        before it, load_state() all of them; save_state() raises while a slot is bound."""
        slots = [int(s) for s in slots]
        ids = [-1 if a is None else int(a) for a in ids]
        scales = [1.0] * len(slots) if scales is None else [float(x) for x in scales]
        if len(ids) != len(slots) or len(scales) != len(slots):
            raise ValueError("set_slot_adapters: one adapter id and one scale per slot")
        sl, ia, sc = np.asarray(slots, np.int32), np.asarray(ids, np.int32), np.asarray(scales, np.float32)
        N.check(N.lib().mp_engine_set_slot_adapters(self._h, sl.ctypes.data, len(slots), ia.ctypes.data, sc.ctypes.data,
                                                    int(_for_start)), "set_slot_adapters")

    def _set_adapters(self, slots, adapters):
        if adapters is None:
            return
        slots = list(slots)
        if len(adapters) != len(slots):
            raise ValueError("adapters: one (id, scale) pair or None per prompt")
        for a in adapters:
            if a is not None and (not isinstance(a, (tuple, list)) or len(a) != 2 or isinstance(a[0], (tuple, list))):
                raise ValueError("adapters: one (id, scale) pair per prompt (stacking adapters is not supported)")
        self.set_slot_adapters(slots, [None if a is None else a[0] for a in adapters],
                               [1.0 if a is None else a[1] for a in adapters], _for_start=True)

    def _set_sampling(self, slots, sampling, for_start=False):
        if sampling is None:
            return
        if len(sampling) != len(slots):
            raise ValueError("sampling: one dict or None per prompt")
        for sl, f in zip(slots, sampling):
            if f is not None:
                self.set_slot_sampling(sl, _for_start=for_start, **f)

    def _set_masks(self, slots, masks):
        if masks is None:
            return
        if len(masks) != len(slots):
            raise ValueError("masks: one mask or None per prompt")
        self.set_slot_masks(list(slots), list(masks), _for_start=True)

    def start(self, prompts, sampling=None, masks=None, adapters=None):
        """sampling (row_sampling engines): one dict of set_slot_sampling fields or None per prompt.
        masks (row_masks engines): one set_slot_masks mask or None per prompt; they constrain the
        prompts' first tokens and stay until changed, whatever the slots ran before.
        adapters (lora_adapters engines): one (adapter id, scale) pair or None (the base model) per
        prompt; without the argument every prompt runs unbound."""
        flat, lens = self._flat(prompts)
        self._n_seq = len(prompts)
        self._set_sampling(range(len(prompts)), sampling, for_start=True)   # start() resets every slot
        self._set_masks(range(len(prompts)), masks)
        self._set_adapters(range(len(prompts)), adapters)
        N.check(N.lib().mp_engine_start(self._h, flat.ctypes.data, lens.ctypes.data, len(prompts)), "start")

    def admit(self, slots, prompts, sampling=None, masks=None, adapters=None):
        """Continuous batching: between decode rounds, prefill `prompts` into the idle sequence slots
        `slots` (slot = micro-batch * mb_size + row); the other slots keep generating.  sampling, masks,
        adapters: as start()."""
        flat, lens = self._flat(prompts)
        self._set_sampling(list(slots), sampling)
        self._set_masks(list(slots), masks)
        self._set_adapters(list(slots), adapters)
        sl = np.asarray(slots, np.int32)
        N.check(N.lib().mp_engine_admit(self._h, sl.ctypes.data, flat.ctypes.data, lens.ctypes.data, len(prompts)),
                "admit")
        self._n_seq = self.n_seq_cap

    def kv_stats(self):
        """Live paged-KV numbers: pool pages, free pages (the `info` dict is a load-time snapshot)."""
        j = N.jcall(N.lib().mp_engine_info, self._h, what="engine info")
        return {"kv_pages": j["kv_pages"], "kv_free_pages": j["kv_free_pages"]}

    def context_shift(self, slots, n_keep, n_discard):
        """Context shift, between decode() calls: for each running slot slots[i], the cached positions
        [n_keep[i], n_keep[i] + n_discard[i]) leave its KV and every later one moves n_discard[i] back: V
        as it is, K rotated by minus n_discard[i] positions on the device, nothing recomputed.
        n_discard > 0 and a multiple of 64; n_keep + n_discard <= slot_position(slot).  The slot's
        position drops by n_discard, n_discard / 64 pages return to the pool, no graph is re-captured.
        Sampler state, masks and adapter bindings stay.  A shifted slot is no prefix-cache hit until it
        is admitted again, and save_state() raises while one is running.  Raises, naming the cause, for
        an idle slot, a violated precondition, mode "mp" / rpc engines and after spec_generate()."""
        sl = np.asarray([int(s) for s in slots], np.int32)
        kp = np.asarray([int(k) for k in n_keep], np.int32)
        nd = np.asarray([int(d) for d in n_discard], np.int32)
        if len(kp) != len(sl) or len(nd) != len(sl):
            raise ValueError("context_shift: one n_keep and one n_discard per slot")
        N.check(N.lib().mp_engine_context_shift(self._h, sl.ctypes.data, len(sl), kp.ctypes.data, nd.ctypes.data),
                "context_shift")

    def set_slot_keep(self, slot: int, n_keep: int):
        """Automatic shifting (Engine(context_shift=True)): the prompt tokens of `slot` a shift keeps
        (-1: the whole prompt) from now on; release() puts the engine's n_keep back."""
        N.check(N.lib().mp_engine_set_slot_keep(self._h, int(slot), int(n_keep)), "set_slot_keep")

    def slot_position(self, slot: int) -> int:
        """Positions the slot's KV holds (prompt + decoded tokens - discarded positions)."""
        return N.check(N.lib().mp_engine_slot_position(self._h, int(slot)), "slot_position")

    def slot_shifts(self, slot: int) -> int:
        """Context shifts of the slot's running sequence."""
        return N.check(N.lib().mp_engine_slot_shifts(self._h, int(slot)), "slot_shifts")

    def release(self, slot: int):
        """Mark a slot idle (its sequence is finished); it can be admitted again."""
        N.check(N.lib().mp_engine_release(self._h, int(slot)), "release")

    def decode(self, k: int):
        return N.jcall(N.lib().mp_engine_decode, self._h, k, what="decode")

    def tokens(self, cap: int | None = None):
        """Generated tokens per sequence; cap: at most that many each (default: all of them)."""
        if cap is None:
            cap = max(N.check(N.lib().mp_engine_tokens_longest(self._h), "tokens"), 1)
        out = np.full((self._n_seq, cap), -1, np.int32)
        n = N.check(N.lib().mp_engine_tokens(self._h, out.ctypes.data, self._n_seq, cap), "tokens")
        return [[t for t in row if t >= 0] for row in out[:, :n].tolist()]

    def logprobs(self):
        """Log-probabilities of the generated tokens (engine built with n_probs != 0): the log-softmax
        of the RAW logits (before penalties, temperature and cuts; llama.cpp's server default).
        Returns per sequence (lp, top_id, top_lp): float32 [n_tokens] aligned with tokens(), and
        [n_tokens][n_probs] alternatives by descending probability (empty with n_probs = -1)."""
        nt = max(int(self.cfg.get("n_probs", 0)), 0)
        # one record per token: the buffers are sized by the longest sequence, the counts are tokens()'s
        counts = [len(t) for t in self.tokens()]
        cap = max(counts + [1])
        lp = np.zeros((self._n_seq, cap), np.float32)
        tid = np.zeros((self._n_seq, cap, nt), np.int32)
        tlp = np.zeros((self._n_seq, cap, nt), np.float32)
        N.check(N.lib().mp_engine_logprobs(self._h, lp.ctypes.data, tid.ctypes.data if nt else None,
                                           tlp.ctypes.data if nt else None, self._n_seq, cap), "logprobs")
        return [(lp[i, :n].copy(), tid[i, :n].copy(), tlp[i, :n].copy()) for i, n in enumerate(counts)]

    def score(self, prompts, n_probs: int = 0):
        """Prompt scoring: per prompt a float32 array of length len(prompt) - 1 whose entry t is
        log p(prompt[t + 1] | prompt[:t + 1]).  With n_probs > 0 returns (lp, top_id, top_lp) per
        prompt instead, the top arrays [len - 1][n_probs].  Prompts are batched over the engine's
        n_mb x mb_size slots; a running generation ends (its KV is overwritten)."""
        res = []
        for g in range(0, len(prompts), self.n_seq_cap):
            grp = prompts[g:g + self.n_seq_cap]
            flat, lens = self._flat(grp)
            rows = int(sum(len(p) - 1 for p in grp))
            lp = np.zeros(max(rows, 1), np.float32)
            tid = np.zeros((max(rows, 1), n_probs), np.int32)
            tlp = np.zeros((max(rows, 1), n_probs), np.float32)
            N.check(N.lib().mp_engine_score(self._h, flat.ctypes.data, lens.ctypes.data, len(grp), n_probs,
                                            lp.ctypes.data, tid.ctypes.data if n_probs else None,
                                            tlp.ctypes.data if n_probs else None), "score")
            o = 0
            for p in grp:
                n = len(p) - 1
                res.append((lp[o:o + n].copy(), tid[o:o + n].copy(), tlp[o:o + n].copy()) if n_probs
                           else lp[o:o + n].copy())
                o += n
        return res

    def idle_slots(self):
        """Sequence slots no running sequence holds (all of them before start())."""
        j = N.jcall(N.lib().mp_engine_info, self._h, what="engine info")
        return list(j["idle_slots"])

    def embed(self, prompts, pooling=None, normalize: bool = True, slots=None):
        """Embeddings of token-id prompts: a list of float32 arrays, [d_model] each, or [len][d_model]
        with pooling "none" (one vector per token).  pooling: "none" | "mean" | "cls" | "last", or
        None for the model's own (its GGUF pooling_type when that is mean, cls or last, otherwise
        "last": in a causal model only the last row has seen the whole prompt).  normalize scales each
        vector to unit L2 length (the zero vector stays zero).  The output RMSNorm is applied, the LM
        head is not run.  Legal before start() and between decode() calls: the prompts run in idle
        slots (`slots`, or as many idle ones as needed, in groups when there are more prompts than
        idle slots), running sequences are untouched and the slots are idle again afterwards."""
        d = self.info["model"]["d_model"]
        prompts = [list(map(int, p)) for p in prompts]
        res = []
        group = len(slots) if slots is not None else max(len(self.idle_slots()), 1)
        for g in range(0, len(prompts), group):
            grp = prompts[g:g + group]
            rq = {"prompts": grp, "normalize": bool(normalize)}
            if pooling is not None:
                rq["pooling"] = pooling
            if slots is not None:
                rq["slots"] = [int(s) for s in slots][:len(grp)]
            rows = [len(p) if pooling == "none" or pooling == 0 else 1 for p in grp]
            out = np.zeros(max(sum(rows), 1) * d, np.float32)
            n = N.check(N.lib().mp_engine_embed(self._h, N.cstr(json.dumps(rq)), out.ctypes.data, out.size), "embed")
            if n != sum(rows) * d:
                raise RuntimeError(f"embed: {n} floats returned, {sum(rows) * d} expected")
            o = 0
            for r in rows:
                v = out[o:o + r * d].copy()
                res.append(v.reshape(r, d) if pooling == "none" or pooling == 0 else v)
                o += r * d
        return res

    def bench(self, prompt_len: int, warmup: int, steps: int):
        return N.jcall(N.lib().mp_engine_bench, self._h, prompt_len, warmup, steps, what="bench")

    def health(self) -> dict:
        """Per-stage heartbeat (items done), link byte counters, ok=False after a pipeline fault."""
        return N.jcall(N.lib().mp_engine_health, self._h, what="engine health")

    def save_state(self, path: str) -> dict:
        """Checkpoint a running generation: every owned stage's KV shard (used positions only),
        decode inputs and sampler step under `path`/, plus the sequences in session.json."""
        return N.jcall(N.lib().mp_engine_save_state, self._h, N.cstr(path), what="save_state")

    def load_state(self, path: str) -> dict:
        """Resume a generation saved by save_state (same model, partition and micro-batch shape);
        decode() then continues exactly where the saved engine stopped."""
        r = N.jcall(N.lib().mp_engine_load_state, self._h, N.cstr(path), what="load_state")
        self._n_seq = r["sequences"]
        return r

    def trace(self, on: bool = True):
        N.check(N.lib().mp_engine_trace(self._h, int(on), None), "trace")

    def write_trace(self, path: str):
        """Chrome-trace JSON (chrome://tracing, Perfetto) of compute/send/recv spans per stage."""
        N.check(N.lib().mp_engine_trace(self._h, 1, N.cstr(path)), "write trace")

    def logits(self, rows: int = 1, vocab: int | None = None):
        vocab = vocab or self.info["model"]["vocab"]
        out = np.zeros((rows, vocab), np.float32)
        N.check(N.lib().mp_engine_logits(self._h, 0, out.ctypes.data, rows), "logits")
        return out


def perplexity_windows(tokens, n_ctx: int, bos: int = -1):
    """llama.cpp's perplexity windows of a token stream: consecutive n_ctx-token pieces (the tail
    that fills no window is dropped), BOS in the first slot when bos >= 0.  Raises when the stream
    has fewer than 2 * n_ctx tokens."""
    n = N.lib().mp_ppl_windows(len(tokens), n_ctx)
    if n < 0:
        raise ValueError(f"perplexity needs at least {2 * n_ctx} tokens, got {len(tokens)}")
    wins = [list(tokens[w * n_ctx:(w + 1) * n_ctx]) for w in range(n)]
    if bos >= 0:
        for w in wins:
            w[0] = bos
    return wins


def perplexity_estimate(window_scores, n_ctx: int) -> dict:
    """Perplexity from the windows' score() arrays (n_ctx - 1 values each): only positions
    [n_ctx / 2, n_ctx - 1) count; err is the standard error of the mean NLL times the PPL."""
    lp = np.ascontiguousarray(np.asarray(window_scores, np.float32).reshape(-1, n_ctx - 1))
    out = (ctypes.c_double * 4)()
    N.check(N.lib().mp_ppl_estimate(lp.ctypes.data, lp.shape[0], n_ctx, out), "perplexity estimate")
    return {"nll": out[0], "ppl": out[1], "err": out[2], "count": int(out[3])}


def device_probe(device: int = 0) -> dict:
    """Halda-style device profile (probe.h): measured HBM read and Q4_K decode-GEMV bandwidth of a
    GPU (device < 0: host memcpy bandwidth, the CPU backend's speed)."""
    out = (ctypes.c_double * 2)()
    N.check(N.lib().mp_device_probe(int(device), out), "device probe")
    return {"hbm_read_gbps": out[0], "gemv_gbps": out[1], "speed": out[1] if out[1] > 0 else out[0]}


def rccl_unique_id_hex() -> str:
    buf = (ctypes.c_uint8 * 128)()
    N.check(N.lib().mp_rccl_unique_id(buf), "rccl unique id")
    return bytes(buf).hex()
