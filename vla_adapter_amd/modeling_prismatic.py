"""Host-side mirror of the reference's model API for the fine-tune hot path, on the native engine.

Keeps:
  * ``OpenVLAForActionPrediction.forward`` - kwargs of prismatic/extern/hf/modeling_prismatic.py:525-544; the
    multimodal branch (:596-655) returns ``PrismaticCausalLMOutputWithPast`` with ``hidden_states`` = tuple of n+1
    ``[B, S, D]`` tensors (HF convention: [0] inputs_embeds ... [n] final-norm output), ``loss=None``, ``logits=None``
    (the reference discards the lm_head output, :680-686; this build never computes it);
  * attributes callers use: ``vision_backbone.get_num_patches()/get_num_images_in_input()/set_num_images_in_input()``
    (:166-193), ``llm_dim`` (:372), ``action_queries``, ``norm_stats``;
  * ``PrismaticVLM.forward`` signature of prismatic/models/vlms/prismatic.py:312-325.
There is no autograd graph: training goes through ``engine.VLAEngine`` (explicit backward kernels).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Dict, Optional, Tuple

import torch

from . import engine as E
from . import ops
from .ops import BF16


@dataclass
class PrismaticCausalLMOutputWithPast:            # modeling_prismatic.py:278-289
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    past_key_values: Any = None
    hidden_states: Optional[Tuple[torch.Tensor, ...]] = None
    attentions: Any = None
    projector_features: Optional[torch.Tensor] = None


class _VisionBackboneView:
    def __init__(self, cfg: E.VLACfg):
        self._cfg = cfg

    def get_num_patches(self) -> int:
        return self._cfg.vit[0].n_patches

    def get_num_images_in_input(self) -> int:
        return self._cfg.n_img

    def set_num_images_in_input(self, n: int) -> None:
        assert n == 1 or self._cfg.fused, "Multi-image inputs require using fused backbone!"   # modeling_prismatic.py:213
        self._cfg.n_img = n


class OpenVLAForActionPrediction:
    def __init__(self, cfg: E.VLACfg, weights: Dict, device="cuda", norm_stats: Optional[dict] = None):
        self.engine = E.VLAEngine(cfg, weights, device)
        self.cfg, self.device = cfg, device
        self.vision_backbone = _VisionBackboneView(cfg)
        self.llm_dim = cfg.llm.d
        self.norm_stats = norm_stats or {}
        self.training = True
        self.serve_latency_hint = None   # predict_actions: None = the engine's default per batch size; True / False force it (tools/bench_serving.py)

    @property
    def action_queries(self) -> torch.Tensor:       # nn.Embedding(64, D).weight in the reference (:375-376)
        return self.engine.head.P.view("action_queries")

    def forward(self, input_ids=None, attention_mask=None, pixel_values=None, labels=None, inputs_embeds=None,
                past_key_values=None, use_cache=None, output_attentions=None, output_hidden_states=None,
                output_projector_features=None, return_dict=None, proprio=None, proprio_projector=None, noisy_actions=None,
                noisy_action_projector=None, diffusion_timestep_embeddings=None, use_film: bool = False):
        if use_film:
            raise NotImplementedError("FiLM (use_film) is outside the accelerated path (off in every shipped script)")
        if past_key_values is not None or inputs_embeds is not None or pixel_values is None or labels is None:
            raise NotImplementedError("only the multimodal training branch (modeling_prismatic.py:596-655) is accelerated")
        assert input_ids.shape[0] == pixel_values.shape[0], "Non-homogenous batch of (text, image) input"
        eng = self.engine
        batch = dict(input_ids=input_ids.to(self.device), labels=labels.to(self.device),
                     attention_mask=attention_mask.to(self.device), pixel_values=pixel_values.to(self.device).contiguous())
        eng.forward_vlm(batch)
        n = self.cfg.llm.n_layers
        hs = tuple(eng.llm.HS[i] for i in range(n + 1)) if (output_hidden_states is None or output_hidden_states) else None
        Np = self.cfg.n_patches
        pf = eng.llm.HS[0][:, 1:Np + 1] if output_projector_features else None
        return PrismaticCausalLMOutputWithPast(loss=None, logits=None, hidden_states=hs, projector_features=pf)

    __call__ = forward

    # ---- batch-1 inference (modeling_prismatic.py:892-972; driver experiments/robot/openvla_utils.py:737-825) ------
    @staticmethod
    def _check_unnorm_key(norm_stats, unnorm_key):                                # modeling_prismatic.py:975-990
        if unnorm_key is None:
            assert len(norm_stats) == 1, ("Your model was trained on more than one dataset, please pass a `unnorm_key` from the "
                                          f"following options to choose the statistics used for un-normalizing actions: {norm_stats.keys()}")
            unnorm_key = next(iter(norm_stats.keys()))
        assert unnorm_key in norm_stats, ("The `unnorm_key` you chose is not in the set of available dataset statistics, "
                                          f"please choose from: {norm_stats.keys()}")
        return unnorm_key

    def get_action_dim(self, unnorm_key=None) -> int:
        return len(self.norm_stats[self._check_unnorm_key(self.norm_stats, unnorm_key)]["action"]["min"])

    def get_action_stats(self, unnorm_key=None):
        return self.norm_stats[self._check_unnorm_key(self.norm_stats, unnorm_key)]["action"]

    def _unnormalize_actions(self, normalized_actions, unnorm_key=None):          # modeling_prismatic.py:784-805
        import numpy as np
        from . import constants as K
        st = self.get_action_stats(unnorm_key)
        if K.ACTION_PROPRIO_NORMALIZATION_TYPE == "bounds":
            mask = st.get("mask", np.ones_like(st["min"], dtype=bool))
            high, low = np.array(st["max"]), np.array(st["min"])
        elif K.ACTION_PROPRIO_NORMALIZATION_TYPE == "bounds_q99":
            mask = st.get("mask", np.ones_like(st["q01"], dtype=bool))
            high, low = np.array(st["q99"]), np.array(st["q01"])
        else:
            raise ValueError("Unsupported action/proprio normalization type detected!")
        return np.where(mask, 0.5 * (normalized_actions + 1) * (high - low + 1e-8) + low, normalized_actions)

    @staticmethod
    def prepare_inference_inputs(input_ids: torch.Tensor, attention_mask: torch.Tensor):
        """_prepare_input_for_action_prediction + _prepare_labels_for_action_prediction (:747-782): append the 64
        placeholder action ids (value 1) and the stop id, fake labels that mark exactly those 64 positions."""
        from . import constants as K
        B, L0 = input_ids.shape
        ids = torch.cat([input_ids, torch.ones(B, K.NUM_TOKENS, dtype=input_ids.dtype, device=input_ids.device),
                         torch.full((B, 1), K.STOP_INDEX, dtype=input_ids.dtype, device=input_ids.device)], dim=-1)
        am = torch.cat([attention_mask, torch.ones(B, ids.shape[-1] - L0, dtype=attention_mask.dtype, device=attention_mask.device)], dim=-1)
        labels = torch.full_like(ids, K.IGNORE_INDEX)
        labels[:, L0:] = K.ACTION_TOKEN_BEGIN_IDX + 1
        labels[:, -1] = K.STOP_INDEX
        return ids, am, labels

    def _load_head(self, action_head, proprio_projector):
        """The mirrors' parameters into the engine, once per (objects, versions); ``True``: the engine's own stay."""
        eng = self.engine
        if action_head is not True:
            sd = action_head.state_dict()
            psd = proprio_projector.state_dict() if (proprio_projector is not None and proprio_projector is not True) else {
                k: v for k, v in eng.head.proprio_views().items()}
            key = (id(action_head), id(proprio_projector), getattr(action_head, "_version", 0), getattr(proprio_projector, "_version", 0))
            if getattr(self, "_loaded_head", None) != key:
                eng.head.load_state_dicts(sd, psd)
                self._loaded_head = key

    def predict_action(self, input_ids=None, unnorm_key=None, proprio=None, proprio_projector=None, action_head=None,
                       noisy_action_projector=None, use_film: bool = False, **kwargs):
        """Same call as the reference (``pixel_values`` / ``attention_mask`` in kwargs, batch 1): returns
        (un-normalised actions ndarray [chunk, action_dim], action hidden states [1, 1, 64, D] of the last layer).
        ``action_head`` / ``proprio_projector``: this package's mirrors (their parameters are loaded into the engine) or
        ``True`` for the parameters the engine already holds (trained in place).  The discrete-token branch
        (``action_head=None`` -> lm_head argmax) is not built."""
        import numpy as np
        if use_film or noisy_action_projector is not None:
            raise NotImplementedError("FiLM / diffusion heads are outside the accelerated path")
        if action_head is None:
            raise NotImplementedError("discrete-token action prediction needs the lm_head (SURVEY 8f-4); pass the L1 regression head")
        assert input_ids.shape[0] == 1, "Generation with batch size > 1 is not currently supported!"     # :700-703
        eng, dev = self.engine, self.device
        self._load_head(action_head, proprio_projector)
        ids, am, labels = self.prepare_inference_inputs(input_ids.to(dev), kwargs["attention_mask"].to(dev))
        use_proprio = proprio_projector is not None and proprio is not None
        assert use_proprio, "the regression head dereferences proprio and its projector (action_heads.py:53-54)"
        pr = torch.as_tensor(np.asarray(proprio), dtype=torch.float32, device=dev).reshape(1, -1)
        batch = dict(input_ids=ids, labels=labels, attention_mask=am.bool(), pixel_values=kwargs["pixel_values"].to(dev).contiguous(),
                     proprio=pr)
        pred = eng.predict(batch)                                                   # [1, chunk, action_dim] bf16
        normalized = pred.reshape(self.cfg.chunk, self.cfg.action_dim).float().cpu().numpy()
        n, Np = self.cfg.llm.n_layers, self.cfg.n_patches
        s0 = Np + input_ids.shape[-1] - 1                                           # NUM_PATCHES + NUM_PROMPT_TOKENS (:856)
        from . import constants as K
        hid = eng.llm.HS[n][:, s0:s0 + K.NUM_TOKENS].reshape(1, 1, K.NUM_TOKENS, -1)
        return self._unnormalize_actions(normalized, unnorm_key), hid

    # ---- batched serving: B observations with prompts of different lengths in one device pass ------------------------------------
    def input_stage(self):
        """The GPUInputStage this model serves through (created on first use): pad id = the tokenizer's, or the last id of a
        vocabulary too small to hold it (the plumbing-size configurations); Normalize per backbone from the vision config."""
        if getattr(self, "_stage", None) is None:
            from . import input_stage as IS
            pad = IS.PAD_TOKEN_ID
            vocab = self.cfg.llm.vocab
            self._stage = IS.GPUInputStage(self.device, pad_token_id=pad if pad < vocab else vocab - 1, backbones=IS.backbone_norms(self.cfg),
                                           image_size=self.cfg.vit[0].img)
        return self._stage

    def predict_actions(self, prompt_ids, *, pixel_values=None, frames_u8=None, center_crop: bool = False, proprio=None,
                        proprio_normalized: bool = False, unnorm_key=None, action_head=True, proprio_projector=True, L=None,
                        return_tensors: bool = False, use_film: bool = False, noisy_action_projector=None, policy_resize: bool = False):
        """predict_action for a batch: B observations, prompts of different lengths, one forward.  Returns (un-normalised actions
        float64 ndarray [B, chunk, action_dim], action hidden states [B, 1, 64, D] of the last layer) - row b is what
        predict_action returns for sample b alone (same layout per row; the bf16 sums of the head run in a batch-dependent order, so
        the values agree to bf16 accuracy, and bit for bit at B == 1 with L = P + 65).

        prompt_ids: list of id lists (the processor's output per sample, untrimmed), or (prompt_flat int64 [n], prompt_off int32
        [B + 1]) tensors; rows are right-padded to L (default: the longest row, P + 65, rounded up to a multiple of 32 -
        input_stage.serve_layout - so that a stream of calls replays few captured shapes).  Host-side prompts with an empty row or
        one that does not fit L raise ValueError; with offsets already on the device nothing is read back, L must be given, and such a
        row comes back as NaN actions (row_ok, include/vla_serve.h).
        Exactly one of pixel_values ([B, C, H, W], already processed) / frames_u8 (raw uint8 frames as GPUInputStage.pixels takes
        them; center_crop: the evaluator's crop first).  Frames that are not at the model's size are resized by the Pillow-bicubic path
        of the input stage ("resize-naive", the processor's own).
        policy_resize (frames_u8 only; with pixel_values: ValueError): the evaluator's resize_image_for_policy
        (experiments/robot/openvla_utils.py:542-565) runs on the frames first - GPUInputStage.policy_frames: a JPEG round trip at quality
        95, then TF's lanczos3 resize with antialiasing to the model's size - and then center_crop and the processor, which is the
        evaluator's order.  Pinned: the round trip, bit for bit, to Pillow / libjpeg-turbo (4:2:0, islow, fancy upsampling); the resize,
        bit for bit, to the float32 numpy rule of tests/policy_image_rule_np.py, which stays within one grey level of Pillow's LANCZOS on
        band-limited frames.  Not pinned (TensorFlow is not available to compare with): TF's own last bits, the order of the two
        resize passes (vertical first here), numpy's sin against glibc's sinf in the weights, and that tf.image.encode_jpeg /
        tf.io.decode_image run libjpeg with exactly those defaults.  H and W of the frames must be multiples of 16.
        proprio [B, Pd]: raw, normalised on the device with norm_stats[key]["proprio"] (the evaluator's normalize_proprio), or
        already normalised (proprio_normalized=True).  action_head / proprio_projector: as in predict_action.
        return_tensors: device tensors (actions f64 [B, chunk, action_dim]) and no host synchronisation on a replayed shape."""
        from . import constants as K
        if use_film or noisy_action_projector is not None:
            raise NotImplementedError("FiLM / diffusion heads are outside the accelerated path")
        if action_head is None:
            raise NotImplementedError("discrete-token action prediction needs the lm_head (SURVEY 8f-4); pass the L1 regression head")
        if (pixel_values is None) == (frames_u8 is None):
            raise ValueError("predict_actions: pass exactly one of pixel_values / frames_u8")
        if policy_resize and frames_u8 is None:
            raise ValueError("predict_actions: policy_resize works on raw frames (frames_u8); pixel_values are already processed")
        if proprio is None or proprio_projector is None:
            raise ValueError("predict_actions: the regression head dereferences proprio and its projector (action_heads.py:53-54)")
        from . import input_stage as IS
        IS.serve_check(prompt_ids, L)                                                # ValueError on a bad host-side prompt, before any work
        eng, dev, stage = self.engine, self.device, self.input_stage()
        tok = stage.serve_tokens(prompt_ids, L)
        self._load_head(action_head, proprio_projector)
        key = self._check_unnorm_key(self.norm_stats, unnorm_key)
        kind = K.ACTION_PROPRIO_NORMALIZATION_TYPE
        B = tok["input_ids"].shape[0]
        if policy_resize:
            frames_u8 = stage.policy_frames(frames_u8)
        px = stage.pixels(frames_u8, center_crop=center_crop) if frames_u8 is not None else pixel_values.to(dev).contiguous()
        if proprio_normalized:
            import numpy as np
            pr = torch.as_tensor(np.asarray(proprio) if not isinstance(proprio, torch.Tensor) else proprio).to(dev, torch.float32)
        else:
            pr = stage.normalize_proprio(proprio, self.norm_stats[key]["proprio"], kind)
        batch = dict(input_ids=tok["input_ids"], labels=tok["labels"], attention_mask=tok["attention_mask"], pixel_values=px,
                     proprio=pr.reshape(B, -1))
        pred = eng.predict(batch, latency_hint=self.serve_latency_hint)              # [B, chunk, action_dim] bf16
        actions = stage.unnormalize_actions(pred, self.get_action_stats(key), kind, row_ok=tok["row_ok"])
        hid = ops.serve_gather_hidden(eng.llm.HS[self.cfg.llm.n_layers], tok["hid_row"], self.cfg.n_patches, K.NUM_TOKENS)
        return (actions, hid) if return_tensors else (actions.cpu().numpy(), hid)

    # ---- serving a token-CE model: greedy action tokens with a key/value cache (prismatic/models/vlas/openvla.py:36-106) -------------
    def generate_actions(self, prompt_ids, *, pixel_values=None, frames_u8=None, center_crop: bool = False, policy_resize: bool = False,
                         unnorm_key=None, max_new_tokens: Optional[int] = None, return_tokens: bool = False, return_tensors: bool = False,
                         use_film: bool = False, do_sample: bool = False, temperature: float = 1.0, top_k: int = 50, top_p: float = 1.0,
                         seed: Optional[int] = None, sample_streams=None, return_logprobs: bool = False):
        """OpenVLA.predict_action for a batch of B observations, for a model trained with the token cross-entropy objective
        (``--objective token_ce``): greedy decoding of T = max_new_tokens action tokens behind every prompt (VLAEngine.generate: one
        prefill, T - 1 cached steps, one device pass), ActionTokenizer.decode_token_ids_to_actions on them (the rule the trainers'
        metrics use: GPUInputStage.decode_token_ids_to_actions, the tokenizer length and bin count of set_objective's defaults), then
        the un-normalisation of openvla.py:99-105 - ``where(mask, 0.5 (a + 1) (q99 - q01) + q01, a)``, which unlike the HF class's
        _unnormalize_actions has no 1e-8 - in float64 on the device.  Returns float64 [B, T / action_dim, action_dim] (an ndarray, or a
        device tensor and no host synchronisation with return_tensors); with return_tokens the pair (actions, tokens int64 [B, T]).

        prompt_ids: a list of id lists - per sample the ids the training collator put in front of the action tokens (a prompt_flat
        row) - or (prompt_flat int64 [n], prompt_off int32 [B + 1]) tensors with the offsets on the host.  Rows are right-padded to a
        multiple of 32.  T defaults to chunk * action_dim, the action ids the collator puts behind the prompt (56 for LIBERO); with
        return_tokens it need not be a multiple of action_dim, and the actions are then None.  There is NO early stop at an
        end-of-sequence id: T tokens are always produced (the reference's `generate` would stop at one; a model trained on action ids
        behind the prompt does not emit it before them).  pixel_values / frames_u8, center_crop, policy_resize: as in predict_actions.
        A LoRA run is served from its merged checkpoint.  By default the choice is the argmax, lowest id among equals.

        do_sample, temperature, top_k, top_p: HF's names with HF's GenerationConfig defaults (the reference passes them through
        **kwargs into `generate`): every token is drawn on the device by the rule of include/vla_sample.h -
        temperature, then top-k (0 switches it off), then top-p, then a Gumbel-max draw whose noise is a function of (seed, stream id
        of the row, step, token id) alone.  seed (an int) is required with do_sample: the same call gives the same tokens.
        sample_streams: B ints, the stream id of every row (default 0 .. B - 1); K samples of one observation are that row repeated
        under K different stream ids (num_return_sequences is not built).  Without do_sample the four settings and the seed must stay
        at their defaults: nothing is silently dropped.  return_logprobs: the log-probability of every emitted token under the
        distribution it was chosen from (greedy: log_softmax of the logits), float32 [B, T] - an ndarray, or a device tensor with
        return_tensors - comes last in the returned tuple."""
        if use_film:
            raise NotImplementedError("generate_actions: FiLM (use_film) is outside the accelerated path")
        if self.engine.fp8_frozen:
            raise NotImplementedError("generate_actions: the fp8 weight path (enable_fp8_frozen) is not covered by the cached decoder")
        sample = None
        if not do_sample:
            if temperature != 1.0 or top_k != 50 or top_p != 1.0 or seed is not None or sample_streams is not None:
                raise ValueError("generate_actions: temperature, top_k, top_p, seed and sample_streams belong to do_sample=True; greedy decoding reads none of them")
        else:
            if isinstance(seed, bool) or not isinstance(seed, int):
                raise ValueError(f"generate_actions: do_sample needs an int seed (draws are reproducible by construction), got {seed!r}")
            try:
                ops.sample_params(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
            except ValueError as e:
                raise ValueError("generate_actions: " + str(e).split(": ", 1)[1]) from None
            sample = dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
        Da = self.cfg.action_dim
        T = self.cfg.chunk * Da if max_new_tokens is None else int(max_new_tokens)
        if T < 1:
            raise ValueError(f"generate_actions: max_new_tokens must be at least 1, got {max_new_tokens}")
        if T % Da and not return_tokens:
            raise ValueError(f"generate_actions: max_new_tokens = {T} is not a multiple of action_dim = {Da}; pass return_tokens=True for the bare tokens")
        if (pixel_values is None) == (frames_u8 is None):
            raise ValueError("generate_actions: pass exactly one of pixel_values / frames_u8")
        if policy_resize and frames_u8 is None:
            raise ValueError("generate_actions: policy_resize works on raw frames (frames_u8); pixel_values are already processed")
        stats = None
        if T % Da == 0:
            if not self.norm_stats or (unnorm_key is None and len(self.norm_stats) != 1) or (unnorm_key is not None and unnorm_key not in self.norm_stats):
                raise ValueError(f"generate_actions: no statistics entry for unnorm_key = {unnorm_key!r}: the model holds {sorted(self.norm_stats)}")
            stats = self.get_action_stats(unnorm_key)
            if "q01" not in stats or "q99" not in stats or len(stats["q01"]) != Da:
                raise ValueError(f"generate_actions: the statistics entry needs q01 and q99 of {Da} dimensions (openvla.py:99-105)")
        from . import input_stage as IS
        lens = IS.serve_prompt_lens(prompt_ids)
        if lens is None:
            raise ValueError("generate_actions: prompt offsets on the device are not accepted (the padded length comes from the lengths)")
        if len(lens) < 1 or min(lens) < 1:
            raise ValueError("generate_actions: every sample needs a prompt of at least one id")
        if sample_streams is not None:
            streams = list(sample_streams)
            if len(streams) != len(lens) or any(isinstance(v, bool) or not isinstance(v, int) for v in streams):
                raise ValueError(f"generate_actions: sample_streams must be B = {len(lens)} ints, got {sample_streams!r}")
            sample["streams"] = streams
        stage, dev = self.input_stage(), self.device
        tok = stage.decode_prompt(prompt_ids, self.cfg.n_patches)
        if policy_resize:
            frames_u8 = stage.policy_frames(frames_u8)
        px = stage.pixels(frames_u8, center_crop=center_crop) if frames_u8 is not None else pixel_values.to(dev).contiguous()
        batch = dict(input_ids=tok["input_ids"], attention_mask=tok["attention_mask"], pixel_values=px, pos=tok["pos"], last_row=tok["last_row"])
        logprobs = None
        if sample is None and not return_logprobs:
            tokens = self.engine.generate(batch, T)                                    # int64 [B, T] on the device
        elif return_logprobs:
            tokens, logprobs = self.engine.generate(batch, T, sample=sample, return_logprobs=True)
            logprobs = logprobs if return_tensors else logprobs.cpu().numpy()
        else:
            tokens = self.engine.generate(batch, T, sample=sample)
        actions = None
        if stats is not None:
            low, high, mask = stage._serve_stats(stats, "bounds_q99")                  # f64 [Da] on the device, mask u8 or None
            a = stage.decode_token_ids_to_actions(tokens).view(tokens.shape[0], T // Da, Da)
            actions = (0.5 * (a + 1.0)) * (high - low) + low                           # numpy's association; every operation rounds on its own
            if mask is not None:
                actions = torch.where(mask.bool(), actions, a)
            if not return_tensors:
                actions = actions.cpu().numpy()
        res = (actions,) + ((tokens,) if return_tokens else ()) + ((logprobs,) if return_logprobs else ())
        return res if len(res) > 1 else actions


@dataclass
class CausalLMOutputWithPast:                     # transformers.modeling_outputs.CausalLMOutputWithPast (what the reference returns)
    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    past_key_values: Any = None
    hidden_states: Optional[Tuple[torch.Tensor, ...]] = None
    attentions: Any = None


class PrismaticVLM:
    """prismatic/models/vlms/prismatic.py:312-481 on the native engine: the fully-multimodal branch of the plain VLM
    forward - ViT(s) -> projector -> [tok0 | patches | tok1..] splice (NO action queries: they belong to
    OpenVLAForActionPrediction) -> Qwen2 stack.  Every argument the native path cannot honour raises; nothing is dropped."""

    def __init__(self, model: OpenVLAForActionPrediction):
        self.model = model

    def forward(self, input_ids=None, attention_mask=None, pixel_values=None, labels=None, inputs_embeds=None,
                past_key_values=None, use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None,
                multimodal_indices=None):
        if input_ids is None or input_ids.shape[1] == 1 or pixel_values is None:
            if past_key_values is not None:
                raise NotImplementedError("cached single-token decoding (prismatic.py:328-342) is outside the accelerated path")
            raise RuntimeError("Invalid `forward()` call!")                      # prismatic.py:344-345
        if inputs_embeds is not None or past_key_values is not None or use_cache:
            raise NotImplementedError("inputs_embeds / past_key_values / use_cache: only the uncached multimodal forward is built")
        if output_attentions:
            raise NotImplementedError("output_attentions: the flash-style attention kernel never materialises the probabilities")
        if return_dict is False:
            raise NotImplementedError("return_dict=False: a CausalLMOutputWithPast is always returned")
        if isinstance(pixel_values, dict):          # {"dino": .., "siglip": ..} (dinosiglip_vit.py:158-170)
            pixel_values = torch.cat([pixel_values["dino"], pixel_values["siglip"]], dim=1)
        B = input_ids.shape[0]
        if multimodal_indices is not None and sorted(int(i) for i in multimodal_indices) != list(range(B)):
            raise NotImplementedError("mixed unimodal/multimodal batches (prismatic.py:424-467) are outside the accelerated path")
        eng, dev = self.model.engine, self.model.device
        if attention_mask is None:
            attention_mask = torch.ones_like(input_ids, dtype=torch.bool)
        batch = dict(input_ids=input_ids.to(dev), attention_mask=attention_mask.to(dev), pixel_values=pixel_values.to(dev).contiguous())
        eng.forward_vlm(batch, action_queries=False)
        n = self.model.cfg.llm.n_layers
        loss = logits = None
        if labels is not None:                      # HF shifted cross-entropy over the vocabulary
            loss, logits = eng.token_ce(labels.to(dev))
        hs = tuple(eng.llm.HS[i] for i in range(n + 1)) if output_hidden_states else None
        return CausalLMOutputWithPast(loss=loss, logits=logits, hidden_states=hs)

    __call__ = forward
