"""AdamW over the one flat parameter buffer of a model, as ONE HIP launch per step (pswin_adamw_flat).

The reference trains with torch.optim.AdamW through mmcv's OptimizerHook (mmdet/apis/train.py:91-112; configs/swin/*.py: lr 1e-4,
betas (0.9, 0.999), weight_decay 0.05).  With every parameter a view of one flat fp32 buffer (dp.GradReducer.flatten_parameters) the
update is a single streaming pass, and the same pass writes the bf16 copy of the updated weights that the next forward pass's
kernels read (backbone._refresh_lowp otherwise makes that copy at the start of every forward).  Element for element the arithmetic
of torch.optim.AdamW; the step counter lives on the device, so `step()` can be captured into a hipGraph and replayed.

The training recipe of the reference's configs -- ``lr_config`` (mmcv's LrUpdaterHook: step policy with a warmup,
configs/_base_/schedules/schedule_1x.py:5-10) and ``optimizer_config.grad_clip`` (mmcv's OptimizerHook -> clip_grad_norm_,
mmdet/utils/optimizer.py:30-32) -- runs on the device too when FlatAdamW is given ``lr_config`` / ``grad_clip`` / ``skip_nonfinite``:
a replayed step then follows the schedule and clips without a host synchronisation (pswin_grad_sumsq -> pswin_adamw_record ->
pswin_adamw_flat_sched, include/pswin.h).  Without those keywords step() is the one launch above, unchanged.
"""
import ctypes
import math

import torch

from ._lib import LrSchedule, PswinError, StepRecord
from .ops import call, ptr


# paramwise_cfg of the reference's Swin configs (configs/swin/mask_rcnn_swin_tiny_patch4_window7_mstrain_480-800_adamw_1x_coco.py:64-67):
# no weight decay on parameters whose name contains one of these keys.  Only 'norm' occurs in this backbone.
REFERENCE_PARAMWISE_CFG = dict(custom_keys={"absolute_pos_embed": dict(decay_mult=0.), "relative_position_bias_table": dict(decay_mult=0.),
                                            "norm": dict(decay_mult=0.)})


def paramwise_groups(named_params, paramwise_cfg, prefix=""):
    """[(name, lr_mult, decay_mult)] by the rule of mmcv's DefaultOptimizerConstructor for ``custom_keys``: the keys are tried
    longest first (ties alphabetically) and the first one that is a substring of the full parameter name decides."""
    keys = (paramwise_cfg or {}).get("custom_keys", {})
    order = sorted(sorted(keys), key=len, reverse=True)
    out = []
    for name, _ in named_params:
        full = f"{prefix}.{name}" if prefix else name
        lr_mult = decay_mult = 1.0
        for k in order:
            if k in full:
                lr_mult, decay_mult = float(keys[k].get("lr_mult", 1.0)), float(keys[k].get("decay_mult", 1.0))
                break
        out.append((name, lr_mult, decay_mult))
    return out


_POLICIES = {"step": 1, "fixed": 0}                                     # PSWIN_LR_STEP / PSWIN_LR_FIXED
_WARMUPS = {None: 0, "constant": 1, "linear": 2, "exp": 3}                # PSWIN_WARMUP_*
_LR_KEYS = {"policy", "by_epoch", "warmup", "warmup_iters", "warmup_ratio", "warmup_by_epoch", "step", "gamma", "min_lr"}


def parse_lr_config(lr_config, iters_per_epoch=None):
    """The merged mmcv ``lr_config`` dict (mmcv 1.2.4 - 1.4.0: 'step' and 'fixed' policies, 'constant' / 'linear' / 'exp' warmup)
    -> a normalised dict (warmup_iters in iterations).  Anything the device schedule does not implement raises PswinError."""
    cfg = dict(lr_config or dict(policy="fixed", by_epoch=False))
    for k in cfg:
        if k not in _LR_KEYS:
            raise PswinError(f"FlatAdamW: lr_config key {k!r} is not supported (supported: {sorted(_LR_KEYS)})")
    policy = cfg.get("policy")
    if not isinstance(policy, str) or policy.lower() not in _POLICIES or policy not in (policy.lower(), policy.title()):
        raise PswinError(f"FlatAdamW: lr_config policy {policy!r} is not supported (only 'step' and 'fixed')")
    policy = policy.lower()
    by_epoch = bool(cfg.get("by_epoch", True))
    warmup = cfg.get("warmup")
    if warmup not in _WARMUPS:
        raise PswinError(f"FlatAdamW: lr_config warmup {warmup!r} is not supported (None, 'constant', 'linear', 'exp')")
    warmup_iters = int(cfg.get("warmup_iters", 0))
    warmup_ratio = float(cfg.get("warmup_ratio", 0.1))
    warmup_by_epoch = bool(cfg.get("warmup_by_epoch", False))
    needs_epoch = (policy == "step" and by_epoch) or (warmup is not None and warmup_by_epoch)
    if needs_epoch and not (isinstance(iters_per_epoch, int) and iters_per_epoch >= 1):
        raise PswinError("FlatAdamW: an epoch-based lr_config needs iters_per_epoch (a positive int)")
    if warmup is not None:
        if warmup_by_epoch:
            warmup_iters *= iters_per_epoch
        if warmup_iters < 1:
            raise PswinError("FlatAdamW: lr_config warmup_iters must be positive")
        if not 0 < warmup_ratio <= 1:
            raise PswinError("FlatAdamW: lr_config warmup_ratio must be in (0, 1]")
    out = dict(policy=policy, by_epoch=by_epoch and policy == "step", iters_per_epoch=iters_per_epoch, warmup=warmup,
               warmup_iters=warmup_iters if warmup is not None else 0, warmup_ratio=warmup_ratio, milestones=[], step_every=0,
               gamma=float(cfg.get("gamma", 0.1)), min_lr=cfg.get("min_lr"))
    if policy == "step":
        step = cfg.get("step")
        if isinstance(step, int) and not isinstance(step, bool) and step > 0:
            out["step_every"] = step
        elif isinstance(step, (list, tuple)) and all(isinstance(x, int) and x > 0 for x in step) and len(step) <= 8 \
                and list(step) == sorted(step):
            out["milestones"] = [int(x) for x in step]
        else:
            raise PswinError(f"FlatAdamW: lr_config step {step!r}: a positive int or up to 8 ascending positive ints")
        if not 0 <= out["gamma"] < math.inf:
            raise PswinError("FlatAdamW: lr_config gamma must be a non-negative number")
        if out["min_lr"] is not None:
            out["min_lr"] = float(out["min_lr"])
    elif "step" in cfg or "gamma" in cfg or "min_lr" in cfg:
        raise PswinError("FlatAdamW: lr_config keys step / gamma / min_lr belong to the 'step' policy")
    return out


def scheduled_lr(sched, base_lr, i):
    """lr of iteration i (0-based, mmcv's runner.iter) for a group whose initial lr is base_lr, in double: the arithmetic of the
    device record (pswin_adamw_record) and of mmcv's StepLrUpdaterHook.get_lr / LrUpdaterHook.get_warmup_lr."""
    lr = base_lr
    if sched["policy"] == "step":
        progress = i // sched["iters_per_epoch"] if sched["by_epoch"] else i
        if sched["milestones"]:
            exp = sum(1 for s in sched["milestones"] if progress >= s)
        else:
            exp = progress // sched["step_every"]
        lr = base_lr * sched["gamma"] ** exp
        if sched["min_lr"] is not None:
            lr = max(lr, sched["min_lr"])
    w = sched["warmup"]
    if w is not None and i < sched["warmup_iters"]:
        frac = i / sched["warmup_iters"]
        if w == "constant":
            lr = lr * sched["warmup_ratio"]
        elif w == "linear":
            lr = lr * (1 - (1 - frac) * (1 - sched["warmup_ratio"]))
        else:
            lr = lr * sched["warmup_ratio"] ** (1 - frac)
    return lr


def parse_grad_clip(grad_clip):
    """mmcv's ``optimizer_config.grad_clip`` (the keywords of clip_grad_norm_): only the 2-norm is implemented."""
    if grad_clip is None:
        return 0.0
    cfg = dict(grad_clip)
    for k in cfg:
        if k not in ("max_norm", "norm_type"):
            raise PswinError(f"FlatAdamW: grad_clip key {k!r} is not supported (max_norm, norm_type)")
    if float(cfg.get("norm_type", 2)) != 2.0:
        raise PswinError(f"FlatAdamW: grad_clip norm_type {cfg['norm_type']!r} is not supported (only the 2-norm)")
    max_norm = cfg.get("max_norm")
    if max_norm is None or not 0 < float(max_norm) < math.inf:
        raise PswinError("FlatAdamW: grad_clip max_norm must be a positive number")
    return float(max_norm)


class FlatAdamW(torch.optim.Optimizer):
    def __init__(self, flat_param, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, model=None, paramwise_cfg=None, prefix="backbone",
                 lr_config=None, iters_per_epoch=None, grad_clip=None, skip_nonfinite=False):
        """flat_param: the nn.Parameter returned by GradReducer.flatten_parameters (its .grad is the flat gradient buffer).
        model: the module whose bf16 Linear shadows are views of one flat bf16 buffer (flatten_parameters(model, torch.bfloat16));
        they are then refreshed by this optimizer's step instead of by the next forward pass.
        paramwise_cfg: mmcv-style ``dict(custom_keys={substring: dict(lr_mult=.., decay_mult=..)})`` (REFERENCE_PARAMWISE_CFG is the
        reference configs'); needs `model` to find every parameter's slot in the flat buffer.  The groups live in a byte map over the
        buffer (one byte per 4 elements) and the update stays ONE launch; `prefix` is the name the model carries inside the detector
        ('backbone' in mmdet's two-stage detectors: the keys are matched against ``backbone.<parameter name>``).
        lr_config: mmcv's merged ``lr_config`` dict (e.g. ``dict(policy='step', warmup='linear', warmup_iters=500, warmup_ratio=0.001,
        step=[8, 11])``), evaluated on the device at every step for the iteration it starts; `lr` is the base lr (mmcv's initial_lr)
        and iters_per_epoch maps epochs to iterations.  grad_clip: ``dict(max_norm=.., norm_type=2)``: the gradient enters the update
        scaled by min(1, max_norm / (norm + 1e-6)) -- the flat gradient buffer itself keeps the UNCLIPPED gradient.  skip_nonfinite:
        a step whose gradient norm is inf / NaN leaves the weights, both moments, the bf16 shadow and Adam's step count alone (the
        iteration counter, and with it the schedule, moves on).  Any of the three switches the step to the scheduled path; the
        counters `iteration` / `skipped`, `lr_tensor` (f32 device scalar: the base group's lr of the last step) and `grad_norm`
        (f32 device scalar: the norm before clipping, 0 without grad_clip / skip_nonfinite) are then kept on the device."""
        if not (isinstance(flat_param, torch.nn.Parameter) and flat_param.dim() == 1 and flat_param.dtype == torch.float32):
            raise PswinError("FlatAdamW wants the one flat fp32 parameter of GradReducer.flatten_parameters")
        if flat_param.numel() % 4 or not flat_param.is_cuda:
            raise PswinError("FlatAdamW: the flat buffer must live on the GPU and hold a multiple of 4 elements")
        super().__init__([flat_param], dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.flat = flat_param
        # the state lives where torch.optim.AdamW(capturable=True) keeps it, under the same keys: state_dict() / load_state_dict()
        # of the two optimizers are interchangeable for the flat parameter
        self.state[flat_param] = dict(step=torch.zeros((), dtype=torch.float32, device=flat_param.device),      # steps taken so far
                                      exp_avg=torch.zeros_like(flat_param.data), exp_avg_sq=torch.zeros_like(flat_param.data))
        self.lowp = None
        self._model = None
        self.group_of = None                 # uint8 [n / 4]: parameter group of every 16-byte granule, or None = one group
        self.group_mults = [(1.0, 1.0)]      # (lr_mult, decay_mult) per group; group 0 = the base group (and the alignment gaps)
        if paramwise_cfg:
            if model is None:
                raise PswinError("FlatAdamW(paramwise_cfg=...) needs `model` to locate the parameters in the flat buffer")
            self._build_groups(model, paramwise_cfg, prefix)
        pair = None if model is None else model.__dict__.get("_flat_pair")
        if pair is not None:
            if pair[0].data_ptr() != flat_param.data_ptr() or pair[1].dtype != torch.bfloat16:
                raise PswinError("FlatAdamW: the model's flat shadow does not belong to this flat parameter")
            import weakref
            self.lowp = pair[1]
            self._model = weakref.ref(model)
            model.__dict__["_lowp_external"] = weakref.ref(self)      # backbone._refresh_lowp: the shadow is kept fresh here ...
            self.sync_lowp()                                          # ... starting in step with the weights as they are now
        self.sched = None
        self.lr_tensor = self.grad_norm = None
        if lr_config is not None or grad_clip is not None or skip_nonfinite:
            self._init_schedule(lr_config, iters_per_epoch, grad_clip, skip_nonfinite)

    def _init_schedule(self, lr_config, iters_per_epoch, grad_clip, skip_nonfinite):
        self.sched = parse_lr_config(lr_config, iters_per_epoch)
        self.max_norm = parse_grad_clip(grad_clip)
        self.skip_nonfinite = bool(skip_nonfinite)
        sc = self.sched
        c = LrSchedule(policy=_POLICIES[sc["policy"]], warmup=_WARMUPS[sc["warmup"]], warmup_iters=sc["warmup_iters"],
                       by_epoch=int(sc["by_epoch"]), iters_per_epoch=sc["iters_per_epoch"] or 0, n_milestones=len(sc["milestones"]),
                       step_every=sc["step_every"], has_min_lr=int(sc["min_lr"] is not None), warmup_ratio=sc["warmup_ratio"],
                       gamma=sc["gamma"], min_lr=sc["min_lr"] or 0.0)
        for q, m in enumerate(sc["milestones"]):
            c.milestones[q] = m
        self._sched_c = c                                              # host structs: copied into the kernel arguments per launch
        k = len(self.group_mults)
        self._lr_mult_c = (ctypes.c_float * k)(*[a for a, _ in self.group_mults])
        self._decay_mult_c = (ctypes.c_float * k)(*[b for _, b in self.group_mults])
        dev = self.flat.device
        self._record = torch.zeros(ctypes.sizeof(StepRecord) // 8, dtype=torch.float64, device=dev)
        words = self._record.view(torch.float32)
        self.lr_tensor = words[StepRecord.lr_base.offset // 4]         # 0-dim views into the record: read without a host sync
        self.grad_norm = words[StepRecord.norm_f.offset // 4]
        self.lr_tensor.fill_(self.lr_at(0))
        self._partials = torch.zeros(1024, dtype=torch.float64, device=dev) if (self.max_norm > 0 or self.skip_nonfinite) else None
        st = self.state[self.flat]
        st["iteration"] = torch.zeros((), dtype=torch.float32, device=dev)  # iterations run (mmcv's runner.iter), skipped ones included
        st["skipped"] = torch.zeros((), dtype=torch.float32, device=dev)    # steps the non-finite guard did not apply
        grp = self.param_groups[0]
        grp["lr_config"] = None if lr_config is None else dict(lr_config)
        grp["grad_clip"] = None if grad_clip is None else dict(grad_clip)
        grp["skip_nonfinite"] = self.skip_nonfinite
        self._recipe = {k: grp[k] for k in ("lr_config", "grad_clip", "skip_nonfinite")}

    def _build_groups(self, model, paramwise_cfg, prefix):
        import numpy as np
        n = self.flat.numel()
        base = self.flat.data_ptr()
        params = list(model.named_parameters())
        gmap = np.zeros(n // 4, dtype=np.uint8)
        for (name, p), (_, lr_mult, decay_mult) in zip(params, paramwise_groups(params, paramwise_cfg, prefix)):
            off = (p.data_ptr() - base) // 4
            if p.data_ptr() < base or off + p.numel() > n or off % 4:
                raise PswinError(f"FlatAdamW: parameter {name} is not a 16-byte aligned view of the flat buffer")
            if (lr_mult, decay_mult) not in self.group_mults:
                self.group_mults.append((lr_mult, decay_mult))
            gmap[off // 4:(off + p.numel() + 3) // 4] = self.group_mults.index((lr_mult, decay_mult))
        if len(self.group_mults) > 8:
            raise PswinError("FlatAdamW: at most 8 distinct (lr_mult, decay_mult) pairs (PSWIN_ADAMW_MAX_GROUPS)")
        if len(self.group_mults) > 1:
            self.group_of = torch.from_numpy(gmap).to(self.flat.device)
        self.param_groups[0]["paramwise_cfg"] = paramwise_cfg

    exp_avg = property(lambda self: self.state[self.flat]["exp_avg"])
    exp_avg_sq = property(lambda self: self.state[self.flat]["exp_avg_sq"])
    step_t = property(lambda self: self.state[self.flat]["step"])
    iteration = property(lambda self: self.state[self.flat].get("iteration"))
    skipped = property(lambda self: self.state[self.flat].get("skipped"))

    def lr_at(self, i, lr_mult=1.0):
        """The lr (double, on the host) the schedule gives a group with this lr_mult at iteration i (0-based; the step that
        follows `iteration` device iterations runs with i = iteration).  Without a schedule: the constant lr."""
        base = float(self.param_groups[0]["lr"]) * lr_mult
        return base if self.sched is None else scheduled_lr(self.sched, base, int(i))

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self.sched is None:
            return
        st = self.state[self.flat]
        dev = self.flat.device
        st["step"] = torch.as_tensor(st["step"], dtype=torch.float32, device=dev).clone()
        if "iteration" not in st:                            # saved without a schedule (torch.optim.AdamW, a plain FlatAdamW)
            st["iteration"] = st["step"].clone()
        if "skipped" not in st:
            st["skipped"] = torch.zeros((), dtype=torch.float32, device=dev)
        for key in ("iteration", "skipped"):
            st[key] = st[key].to(dtype=torch.float32, device=dev).reshape(())
        grp = self.param_groups[0]                           # the recipe is this optimizer's (as its parameter groups are)
        for key in ("lr_config", "grad_clip", "skip_nonfinite"):
            grp[key] = self._recipe[key]

    @torch.no_grad()
    def sync_lowp(self):
        """Refresh the bf16 shadow from the master weights now.  Needed by hand only where the model cannot notice a change by
        itself: weights edited between REPLAYS of a captured step (no Python runs there), or through raw pointers / ``p.data``
        without model.mark_weights_changed().  Everything PyTorch tracks (load_state_dict, nn.init, another optimizer's step) is
        detected by the next forward pass (backbone._weights_signature)."""
        if self.lowp is not None:
            self.lowp.copy_(self.flat.data)
            m = self._model() if getattr(self, "_model", None) is not None else None
            if m is not None:
                m.__dict__["_lowp_sig"] = m._weights_signature()

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise PswinError("FlatAdamW does not take a closure")
        g = self.flat.grad
        if g is None:
            return None
        if g.dtype != torch.float32 or not g.is_contiguous() or g.numel() != self.flat.numel():
            raise PswinError("FlatAdamW: the gradient must be the flat fp32 gradient buffer")
        grp = self.param_groups[0]
        st = self.state[self.flat]
        if st["step"].dtype != torch.float32 or not st["step"].is_cuda:                   # (a state dict saved by torch's non-capturable AdamW)
            st["step"] = torch.as_tensor(float(st["step"]), dtype=torch.float32, device=self.flat.device)
        if self.sched is not None:
            return self._step_scheduled(g, grp, st)
        st["step"] += 1.0
        if self.group_of is None:
            call("pswin_adamw_flat", self.flat, ptr(self.flat.data), ptr(g), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self.lowp),
                 self.flat.numel(), float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1]), float(grp["eps"]),
                 float(grp["weight_decay"]), ptr(self.step_t),
                 algo_bytes=self.flat.numel() * (28 + (2 if self.lowp is not None else 0)))
            return None
        import ctypes
        k = len(self.group_mults)
        lr_m = (ctypes.c_float * k)(*[a for a, _ in self.group_mults])
        dc_m = (ctypes.c_float * k)(*[b for _, b in self.group_mults])
        call("pswin_adamw_flat_groups", self.flat, ptr(self.flat.data), ptr(g), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self.lowp),
             self.flat.numel(), ptr(self.group_of), k, ctypes.cast(lr_m, ctypes.c_void_p), ctypes.cast(dc_m, ctypes.c_void_p),
             float(grp["lr"]), float(grp["betas"][0]), float(grp["betas"][1]), float(grp["eps"]), float(grp["weight_decay"]),
             ptr(self.step_t), algo_bytes=self.flat.numel() * (28.25 + (2 if self.lowp is not None else 0)))
        return None

    def _step_scheduled(self, g, grp, st):
        """sum of squares (with clipping / the guard) -> one-workgroup record (counters, norm, clip coefficient, lr per group) ->
        the update reading the record.  Nothing here reads a device value on the host: the three launches capture as they are."""
        n = self.flat.numel()
        partials = None
        if self._partials is not None:
            call("pswin_grad_sumsq", self.flat, ptr(g), n, ptr(self._partials), algo_bytes=n * 4)
            partials = ptr(self._partials)
        grouped = self.group_of is not None
        k = len(self.group_mults) if grouped else 0
        call("pswin_adamw_record", self.flat, partials, ctypes.addressof(self._sched_c), float(grp["lr"]), k,
             ctypes.addressof(self._lr_mult_c) if grouped else None, self.max_norm, int(self.skip_nonfinite), ptr(st["step"]),
             ptr(st["iteration"]), ptr(st["skipped"]), ptr(self._record))
        call("pswin_adamw_flat_sched", self.flat, ptr(self.flat.data), ptr(g), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self.lowp),
             n, ptr(self.group_of), k, ctypes.addressof(self._decay_mult_c) if grouped else None, float(grp["betas"][0]),
             float(grp["betas"][1]), float(grp["eps"]), float(grp["weight_decay"]), ptr(self._record),
             algo_bytes=n * ((28.25 if grouped else 28) + (2 if self.lowp is not None else 0)))
        return None
