"""Experiment configuration with the reference's surface:

  * ``get_cfg_defaults()`` — the keys and defaults of the reference's ``defaults.py:7-37`` (a yacs ``CfgNode``
    there; yacs is not installed here, so ``CfgNode`` below re-implements the subset the reference uses:
    attribute/item access, ``clone``, ``merge_from_file`` that rejects unknown keys and mismatched types like
    yacs does, ``freeze``).
  * ``ExperimentConfig(folder, device=None, remove=False, resume=False, run_prefix='run', tensorboard=True)``
    — ``experiment_config.py:12-51``: run-directory numbering, summary writer, ``<folder>/config.yml`` merged
    over the defaults, LOSS_CLIP validation, every key copied onto the instance, ``device``/``gpu_id``.

Keys added by this build (all optional, defaults reproduce the reference): BATCH_SIZE (the reference
hard-codes 16, train_q_network.py:98), NUM_WORKERS (8), COMPUTE_DTYPE ('bf16' | 'f32' | 'bf16x3': f32 storage, GEMMs as split bf16 x 3), NUM_FRAMES (0 = the
reference's rule: 4 if PANORAMA or PREVIOUS_IMAGES else 1), SYNTHETIC_DATA (train on generated frames), DEVICE_RESIDENT_DATA ('auto' | 'on' | 'off': keep a decoded-frame shard
dataset in HBM and gather minibatches on the device), SHARD_INPUT ('stream' | 'dataloader': how a shard dataset that is NOT
resident reaches the GPU — memory-mapped shards + native gather into pinned double buffers, or torch's DataLoader),
HOST_GATHER_THREADS, SYNC_BN (ARCHITECTURE='basic' on several GPUs: global BatchNorm
statistics, so N ranks equal the reference's single big batch; default True), DETERMINISTIC (run-to-run bit-identical
updates — the reference's cudnn.deterministic = True, train_q_network.py:88-89 — at a small throughput cost), LOSS_KIND ('l2' = the reference's half
squared TD error, train_q_network.py:167; 'huber' = smooth-L1, the option archs/HabitatDQNMultiAction.py:25 leaves open),
PRETRAINED_WEIGHTS (path of a torchvision resnet18 state_dict: the reference builds models.resnet18(pretrained=True),
archs/HabitatDQNMultiAction.py:11, which needs a download this build cannot make), BOOTSTRAP_CHECKPOINT (the file the
BOOTSTRAP branch loads; default = the path hard-coded at train_q_network.py:202), PRIORITIZED_REPLAY (False: draw every
minibatch by priority — prioritized experience replay, sampled and updated on the GPU — instead of in shuffled epochs; the TD
branch on an HBM-resident decoded-frame shard dataset only), PER_ALPHA (0.6: priority exponent, p = (|TD error| + 1e-6)^alpha),
PER_BETA (0.4: importance-sampling exponent at step 0, annealed linearly to 1.0 at NUM_STEPS), AUG_SHIFT_PAD (0 = off, 0..32: random
shift augmentation — every update shows each sample padded by this many edge-replicated pixels and cropped at a random offset, one
draw per sample shared by its frames and by s and s', fused into the input pack on the GPU), AUG_FLIP (False: mirror each sample
left-right with probability 1/2, s and s' together), AUG_FLIP_ACTIONS ([1, 2]: the two action labels a mirror exchanges — turn left
and turn right; from dataloaders/gibson.py:76 and habitat_test_env.py:242 under Habitat-API 0.1.3's STOP 0 / FORWARD 1 / LEFT 2 /
RIGHT 3, unverified here, hence a key), AUG_BRIGHTNESS, AUG_CONTRAST, AUG_SATURATION (0.0 = off, each in [0, 1]: colour jitter — the
half-width J of a uniform factor range [1 - J, 1 + J] as torchvision's ColorJitter; one factor triple per update and sample, shared by
its frames and by s and s', applied to the uint8 pixels in integer arithmetic, saturation then brightness then contrast about
mid-grey 128, inside the same input pack on the GPU), AUG_ZOOM (0.0 = off, in [0, 0.5]: random zoom — a window whose side is uniform in
[1 - AUG_ZOOM, 1] of the frame's, at a uniform position inside the frame, resampled back to 224 x 224 with an integer bilinear filter
inside the same input pack; a magnification of at most 2, never a zoom-out; one window per update and sample, shared by its frames
and by s and s'), AUG_ZOOM_ASPECT (False: the window's two sides are drawn independently, each from [1 - AUG_ZOOM, 1], which also
stretches the picture; needs AUG_ZOOM > 0), AUG_ROTATE (0.0 = off, in [0, 30] degrees: random rotation, camera roll — an angle uniform in
[-AUG_ROTATE, AUG_ROTATE] about the picture's centre, one per update and sample, shared by its frames and by s and s'; composed with
the zoom window into one affine map and resampled with the same integer bilinear filter by a tiled pack kernel on the GPU; pixels
that fall outside the frame replicate its edge; costs one packed-frame buffer of 2 * BATCH_SIZE * NUM_FRAMES * 115 * 115 * 16 elements),
GRAD_CLIP_NORM (0.0 = off; > 0: the whole gradient is rescaled so that its global L2 norm
is at most this, torch.nn.utils.clip_grad_norm_: coef = min(1, max_norm / (norm + 1e-6)), norm and coefficient computed on the GPU
and never read back for the update), WEIGHT_DECAY (0.0: decoupled, as torch.optim.AdamW: p <- p * (1 - lr * wd) in front of the
Adam update, over every trainable element; resnet.fc, which never receives a gradient, stays untouched), LR_WARMUP_STEPS (0:
the rate of update t, the 1-based sample_number, is multiplied by min(1, t / W)), LR_SCHEDULE ('constant' | 'linear' | 'cosine': after
the warm-up the rate goes from LEARNING_RATE to LEARNING_RATE * LR_FINAL_FRACTION at NUM_STEPS, progress = clamp((t - W) /
(NUM_STEPS - W), 0, 1); cosine is f + (1 - f) * (1 + cos(pi * progress)) / 2), LR_FINAL_FRACTION (0.0), CQL_ALPHA (0.0 = off; > 0:
conservative Q-learning for training from logged data, Kumar et al. 2020 — CQL_ALPHA * (logsumexp_a Q(s, .) - Q(s, a_data)), averaged
like the TD loss, is added to it inside the loss launch on the GPU, which pulls down the values of actions the data never shows;
1.0 is the usual discrete setting; the TD branch with more than one action column only), TARGET_TAU (0.0 = off, the reference's hard
target copy every TARGET_UPDATE_INTERVAL updates; in (0, 1]: soft / Polyak target updates — after every optimiser step the target
weights move as target <- target + TARGET_TAU * (online - target), inside the Adam launch on the GPU, in an f32 copy of all
parameters from which the target network's weights are folded in front of every update; TARGET_UPDATE_INTERVAL is then unused;
BatchNorm running statistics are copied from the online network, not averaged; 0.005 is the usual setting; the checkpoint gains
`target_state_dict`; the TD branch only), VAL_DATASET ('' = off: the held-out set of the validation pass the reference reserves
and never fills, train_q_network.py:183-186,240 — a path as DATASET takes it, or 'synthetic', a SyntheticTupleDataset of 1024 tuples
seeded with SEED + 1), VAL_INTERVAL (0 = off; > 0: after every update t with t % VAL_INTERVAL == 0, in front of that update's
checkpoint, rank 0 walks the validation set in index order in batches of BATCH_SIZE, the last short one included, without
augmentation or importance weights — forward passes only, the metric sums kept on the GPU and read back once per pass — and logs
avg_q_loss/val, td_abs_error/val, q_data/val, q_max/val, td_target/val, cql_penalty/val, action_agreement/val and the per-category
avg_q_loss_cat<c>/val; the TD branch only; needs VAL_DATASET), VAL_BATCHES (0 = the whole validation set; > 0: its first
VAL_BATCHES batches), N_STEP (1 = off, the reference's one-step target; 2 .. 16: n-step returns — the target of a sampled row is the
N_STEP-fold composition of the one-step backup along the row's chain in the logged data, the row that follows row r being the row
whose first `before` frame is r's first `after` frame, found in the shard index as it is; rewards, terminals and the discount
gamma^m are folded by one launch on the GPU per update and s' is the `after` frame of the last of the m <= N_STEP rows the chain
provides, so every sample still costs one s' forward; no importance correction: with non-negative rewards the target is a lower
bound of the optimal value; the sampled rows are those of N_STEP 1 under the same seed; the TD branch without LINEAR on a
decoded-frame shard dataset held in full in HBM on every rank; validation stays one-step), MC_RETURN_FLOOR (False = off; True: the
bootstrapped target of a sampled row is floored by the discounted return G the logged data itself obtained from that row to the end
of its chain, y <- max(y, G) in front of the rect clip — lower-bound Q-learning; G is a table over all rows, built once at start on
the GPU by pointer doubling at GAMMA, per category; with N_STEP > 1 the floor is still the sampled row's whole-chain return; logs
mc_floor_share/train, the share of targets the floor raises, and q_minus_return/train, the mean of Q(s, a_data) - G; the same
configurations as N_STEP > 1: the TD branch without LINEAR on a decoded-frame shard dataset held in full in HBM on every rank;
nothing goes into checkpoints, validation is unchanged), CQL_CALIBRATED (False = off; True: calibrated conservative Q-learning,
Cal-QL — the penalty's logsumexp runs over max(Q(s, a), G) with the same table G, so the penalty stops pushing values below what
the data achieved; needs CQL_ALPHA > 0 and what MC_RETURN_FLOOR needs; logs the same two scalars), IQL_EXPECTILE (0.0 = off; in
[0.5, 1): implicit Q-learning, Kostrikov et al. 2022 — the network gets a value head V(s), five more rows of its Q layer stored as
value.weight / value.bias, fitted by expectile regression at IQL_EXPECTILE to the target network's Q(s, a_data), and Q(s, a_data) is
regressed on r + GAMMA (1 - t) V(s') where Double DQN takes Q_target(s', argmax_a Q(s', .)): no action outside the logged data is
evaluated; 0.7 is the usual setting, 0.5 fits the mean; the target pass runs over s instead of s', so an update costs what it did;
logs iql_v_loss/train and iql_advantage/train, the mean of Q_target(s, a_data) - V(s); the TD branch with three action columns and
without LINEAR; not together with CQL_ALPHA, CQL_CALIBRATED or MC_RETURN_FLOOR; composes with N_STEP, PRIORITIZED_REPLAY, AUG_*
and TARGET_TAU; checkpoints keep the reference's keys and shapes and carry the head under a key of their own, `value_head`;
validation adds iql_v_loss/val, iql_advantage/val, iql_q_loss/val and the rest of the value head's held-out metrics to the one-step
Double-DQN metrics on the Q columns), DISTRIBUTIONAL / KL_BACKWARDS / LOG_SIGMA (the
reference's keys, defaults.py:34-36, all False = off) and DIST_SIGMA_MIN (0.1; in [1e-4, 10]): Gaussian distributional Q-learning —
the network gets a spread head, one more row of its Q layer per Q column stored as spread.weight / spread.bias, so that every
(category, action) carries a mean (the Q column, as ever) and a variance sigma^2 + DIST_SIGMA_MIN^2 with sigma = softplus(rho), or
exp(rho) clamped to rho in [-8, 4] under LOG_SIGMA; the loss is the KL divergence between that Gaussian at the data action and the
Double-DQN backup's, N(r + GAMMA (1 - t) mean', max((GAMMA (1 - t))^2 var', DIST_SIGMA_MIN^2)) from the target network at the online
arg-max of the means — KL(backup || prediction), or KL(prediction || backup) under KL_BACKWARDS; an update keeps its three forward
passes and one backward, only the loss launch differs; avg_q_loss/train is the KL objective, dist_sigma/train the mean predicted
sigma at the data action and dist_z2/train the mean squared standardised error (1 when calibrated); model.distribution(frames)
returns (B, C, A, 2) = mean and variance, what the reference's visualize_value.py indexes; KL_BACKWARDS or LOG_SIGMA without
DISTRIBUTIONAL is refused (no effect); the TD branch without LINEAR and with LOSS_KIND l2; not together with CQL_ALPHA,
CQL_CALIBRATED, MC_RETURN_FLOOR or IQL_EXPECTILE (deliberately out of scope); composes with N_STEP, PRIORITIZED_REPLAY, AUG_*,
TARGET_TAU, ONE_ACTION, both architectures and N ranks; checkpoints keep the reference's keys and shapes and carry the head, its
Adam moments and under TARGET_TAU its target rows under a key of their own, `spread_head`; validation adds dist_kl/val,
dist_sigma/val, dist_z2/val, dist_nll/val, dist_coverage/val — 0.683 when the spread is calibrated — and the backup's and the greedy
action's sigma),
BCQ_THRESHOLD (-1.0 = off; tau in [0, 1), 0.3 in the paper), BCQ_BC_WEIGHT (1.0; > 0) and BCQ_LOGIT_REG (0.01; >= 0): discrete
batch-constrained Q-learning (BCQ, Fujimoto et al. 2019) — the network gets a policy head, one more row of its Q layer per action
stored as policy.weight / policy.bias, whose logits i(a) are fitted to the logged action by cross-entropy (weight BCQ_BC_WEIGHT,
plus BCQ_LOGIT_REG times the mean squared logit), and the Double-DQN target's arg-max at s' runs only over the actions with
pi_b(a | s') / max_a' pi_b(a' | s') > tau under the online head; 0.0 trains the head and constrains nothing, values near 1 clone the
behaviour with a learned value; an update keeps its three forward passes and one backward, only the loss launch differs;
bcq_bc_loss/train is the mean cross-entropy, bcq_constrained_share/train the share of targets whose action the constraint changed
and bcq_accuracy/train how often the head's arg-max is the logged action; model.behaviour(frames) returns the probabilities,
model.constrained_q(frames, tau) the Q values with the disallowed actions at -inf; BCQ_BC_WEIGHT or BCQ_LOGIT_REG away from their
defaults without BCQ_THRESHOLD is refused (no effect); the TD branch without LINEAR, VALUE_LEARNING and ONE_ACTION; not together
with CQL_ALPHA, CQL_CALIBRATED, MC_RETURN_FLOOR, IQL_EXPECTILE or DISTRIBUTIONAL (deliberately out of scope); composes with N_STEP,
PRIORITIZED_REPLAY, AUG_* (AUG_FLIP exchanges the action labels before the loss, so the behaviour target follows it), TARGET_TAU,
LOSS_KIND huber, both architectures and N ranks; checkpoints keep the reference's keys and shapes and carry the head and its Adam
moments under a key of their own, `policy_head`; validation adds bcq_bc_loss/val, bcq_accuracy/val, bcq_constrained_share/val,
bcq_policy_agreement/val — the constrained policy at s against the logged action — and the rest of the policy head's held-out metrics).
"""
from __future__ import annotations

import copy
import json
import os
import re
import shutil

import yaml

VALID_VALUES = {"LOSS_CLIP": ["sigmoid", "rect", "none"],  # experiment_config.py:10
                "LOSS_KIND": ["l2", "huber"],
                "LR_SCHEDULE": ["constant", "linear", "cosine"]}


class CfgNode(dict):
    """Minimal yacs-compatible node (flat: the reference's config has no nesting)."""

    def __init__(self, init=None):
        super().__init__(init or {})
        object.__setattr__(self, "_frozen", False)

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        if self._frozen:
            raise AttributeError(f"Attempted to set {k} to {v}, but CfgNode is immutable")
        self[k] = v

    def clone(self):
        c = CfgNode(copy.deepcopy(dict(self)))
        return c

    def freeze(self):
        object.__setattr__(self, "_frozen", True)

    def defrost(self):
        object.__setattr__(self, "_frozen", False)

    def merge_from_file(self, path):
        with open(path) as f:
            loaded = yaml.safe_load(f) or {}
        self.merge_from_dict(loaded)

    def merge_from_dict(self, loaded):
        for k, v in loaded.items():
            if k not in self:
                raise KeyError(f"Non-existent config key: {k}")
            self[k] = _check_and_coerce(v, self[k], k)

    def dump(self):
        return yaml.safe_dump(dict(self))

    def __str__(self):
        return "\n".join(f"{k}: {self[k]!r}" if isinstance(self[k], str) else f"{k}: {self[k]}" for k in sorted(self))


def _check_and_coerce(new, old, key):
    """yacs' _check_and_coerce_cfg_value_type: same type, or int<->float / tuple<->list casts, else error."""
    if type(new) is type(old):
        return new
    if isinstance(old, float) and isinstance(new, int) and not isinstance(new, bool):
        return float(new)
    if isinstance(old, int) and not isinstance(old, bool) and isinstance(new, float) and float(new).is_integer():
        return int(new)
    if isinstance(old, (list, tuple)) and isinstance(new, (list, tuple)):
        return type(old)(new)
    raise ValueError(f"Type mismatch ({type(old)} vs. {type(new)}) with values ({old} vs. {new}) for config key: {key}")


def get_cfg_defaults() -> CfgNode:
    """defaults.py:7-37 (+ this build's optional keys)."""
    c = CfgNode()
    c.PANORAMA = True
    c.SEED = 0
    c.TRAIN_ON_GROUND_TRUTH = False
    c.DATASET = "none"
    c.SUB_DATASET = "none"
    c.CLASS_LABEL = "toilet"
    c.LOSS_CLIP = "none"
    c.ARCHITECTURE = "basic"
    c.RANDOM_ACTIONS = False
    c.ONE_ACTION = False
    c.SEMANTIC_REWARDS = False
    c.DETECTION_REWARDS = False
    c.REMOVE_BEFORE_REWARD = False
    c.USE_INVERSE_ACTIONS = False
    c.VALUE_LEARNING = False
    c.PREVIOUS_IMAGES = False
    c.GAMMA = 0.9
    c.BOOTSTRAP = False
    c.LINEAR = False
    c.LEARNING_RATE = 1e-3
    c.NUM_STEPS = int(1e5)
    c.TARGET_UPDATE_INTERVAL = int(8e3)
    c.CHECKPOINT_INTERVAL = int(2e3)
    c.ACTION_HIDDEN_LAYERS = 1
    c.GUMBEL_TEMP = 0.1
    c.CONFIDENCE_REWARD = False
    c.DISTRIBUTIONAL = False
    c.KL_BACKWARDS = False
    c.LOG_SIGMA = False
    c.VISUALIZATION_DATA_ROOT = ""
    # --- added by this build ---
    c.BATCH_SIZE = 16
    c.NUM_WORKERS = 8
    c.COMPUTE_DTYPE = "bf16"
    c.NUM_FRAMES = 0
    c.SYNTHETIC_DATA = False
    c.SYNC_BN = True
    c.DEVICE_RESIDENT_DATA = "auto"
    c.RANK_SHARDED_DATA = True    # resident data on several GPUs: every rank holds the frames of ITS samples of the epoch, not a full copy
    c.SHARD_INPUT = "stream"      # decoded-frame shards that are not resident: 'stream' (HostFrameStream) | 'dataloader'
    c.HOST_GATHER_THREADS = 0     # native threads of the streaming path's frame gather (0 = min(16, cores / 2))
    c.DETERMINISTIC = False
    c.LOSS_KIND = "l2"
    c.PRETRAINED_WEIGHTS = ""
    c.BOOTSTRAP_CHECKPOINT = "logs/trained_gt_0.99/models/epoch99.torch"
    c.PRIORITIZED_REPLAY = False  # sample minibatches by priority (PER, on the device) instead of shuffled epochs
    c.PER_ALPHA = 0.6             # priority exponent: p = (|TD error| + 1e-6) ^ PER_ALPHA
    c.PER_BETA = 0.4              # importance-sampling exponent at step 0, annealed linearly to 1.0 at NUM_STEPS
    c.AUG_SHIFT_PAD = 0           # random-shift augmentation: pad by this many replicated edge pixels, crop at a random offset (0 = off, <= 32)
    c.AUG_FLIP = False            # random left-right mirror of a sample (s and s' together), with its action label exchanged
    c.AUG_FLIP_ACTIONS = [1, 2]   # the two action labels a mirror exchanges (turn left, turn right)
    c.AUG_BRIGHTNESS = 0.0        # colour jitter: brightness factor uniform in [1 - AUG_BRIGHTNESS, 1 + AUG_BRIGHTNESS] (0 = off, <= 1)
    c.AUG_CONTRAST = 0.0          # contrast factor about mid-grey 128, uniform in [1 - AUG_CONTRAST, 1 + AUG_CONTRAST] (0 = off, <= 1)
    c.AUG_SATURATION = 0.0        # saturation factor, uniform in [1 - AUG_SATURATION, 1 + AUG_SATURATION] (0 = off, <= 1)
    c.AUG_ZOOM = 0.0              # random zoom: the window's side is uniform in [1 - AUG_ZOOM, 1] of the frame's, resampled to 224 (0 = off, <= 0.5)
    c.AUG_ZOOM_ASPECT = False     # draw the window's two sides independently (a stretch); needs AUG_ZOOM > 0
    c.AUG_ROTATE = 0.0            # random rotation about the picture's centre: the angle is uniform in [-AUG_ROTATE, AUG_ROTATE] degrees (0 = off, <= 30)
    c.GRAD_CLIP_NORM = 0.0        # > 0: rescale the gradient to this global L2 norm at most (clip_grad_norm_, on the GPU); 0 = off
    c.WEIGHT_DECAY = 0.0          # decoupled weight decay (AdamW): p <- p * (1 - lr * WEIGHT_DECAY) in front of the Adam update
    c.LR_WARMUP_STEPS = 0         # the learning rate of update t is multiplied by min(1, t / LR_WARMUP_STEPS)
    c.LR_SCHEDULE = "constant"    # 'constant' | 'linear' | 'cosine': from LEARNING_RATE to LEARNING_RATE * LR_FINAL_FRACTION at NUM_STEPS
    c.LR_FINAL_FRACTION = 0.0
    c.CQL_ALPHA = 0.0             # > 0: conservative Q-learning penalty CQL_ALPHA * (logsumexp_a Q(s, .) - Q(s, a_data)) in the loss launch; 0 = off
    c.TARGET_TAU = 0.0            # in (0, 1]: soft target updates target <- target + TARGET_TAU * (online - target) after every optimiser step; 0 = hard copies
    c.VAL_DATASET = ""            # held-out validation set: a path as DATASET takes it, or 'synthetic' (seeded with SEED + 1); '' = off
    c.VAL_INTERVAL = 0            # > 0: a validation pass on rank 0 after every update t with t % VAL_INTERVAL == 0; 0 = off
    c.VAL_BATCHES = 0             # > 0: only the first VAL_BATCHES batches of the validation set; 0 = the whole set
    c.MC_RETURN_FLOOR = False     # True: y <- max(y, G), G the Monte-Carlo return of the sampled row along its chain (a table built on the GPU at start)
    c.CQL_CALIBRATED = False      # True: Cal-QL — the CQL penalty's logsumexp over max(Q, G); needs CQL_ALPHA > 0
    c.IQL_EXPECTILE = 0.0         # in [0.5, 1): implicit Q-learning — a value head fitted to Q_target(s, a_data) at this expectile, the bootstrap from V(s'); 0 = off
    c.DIST_SIGMA_MIN = 0.1        # DISTRIBUTIONAL: the floor of the predicted and of the backed-up standard deviation, in [1e-4, 10]
    c.BCQ_THRESHOLD = -1.0        # in [0, 1): discrete BCQ — the target's arg-max only over actions with pi_b(a|s') / max pi_b > this, pi_b a policy head fitted to the logged actions; 0 = head on, nothing constrained; -1 = off
    c.BCQ_BC_WEIGHT = 1.0         # BCQ_THRESHOLD: the weight of the behaviour head's cross-entropy in the loss, > 0
    c.BCQ_LOGIT_REG = 0.01        # BCQ_THRESHOLD: the weight of the mean squared behaviour logit (Fujimoto's regulariser), >= 0
    c.N_STEP = 1                  # 2 .. 16: n-step returns along each sampled row's chain in the logged data, folded on the GPU; 1 = off
    return c


class JsonlWriter:
    """Stand-in for tensorboardX.SummaryWriter when it is not installed: same add_scalar/add_image/close calls,
    scalars appended to <log_dir>/scalars.jsonl."""

    def __init__(self, log_dir, comment=""):
        os.makedirs(log_dir, exist_ok=True)
        self.log_dir = log_dir
        self._f = open(os.path.join(log_dir, "scalars.jsonl"), "a")

    def add_scalar(self, tag, value, global_step=None):
        self._f.write(json.dumps({"tag": tag, "value": float(value), "step": global_step}) + "\n")
        self._f.flush()

    def add_image(self, *a, **k):
        pass

    def close(self):
        self._f.close()


def _make_writer(log_dir):
    try:
        from tensorboardX import SummaryWriter  # the reference's writer (experiment_config.py:5,32)
        return SummaryWriter(log_dir=log_dir, comment=log_dir)
    except ImportError:
        try:
            from torch.utils.tensorboard import SummaryWriter
            return SummaryWriter(log_dir=log_dir, comment=log_dir)
        except Exception:
            return JsonlWriter(log_dir)


class ExperimentConfig:
    """experiment_config.py:12-51."""

    def __init__(self, folder, device=None, remove=False, resume=False, run_prefix="run", tensorboard=True):
        import torch
        self.folder = folder
        if remove:  # :16-17  rm -r <folder>/<run_prefix>*
            for f in os.listdir(folder):
                if f.startswith(run_prefix):
                    p = os.path.join(folder, f)
                    shutil.rmtree(p) if os.path.isdir(p) else os.remove(p)
        self.files = sorted(os.listdir(folder))  # :19  (`ls` order)
        max_run = 0
        for f in self.files:  # :21-24  last match wins
            m = re.search(f"^{run_prefix}(\\d+)$", f)
            if m:
                max_run = int(m[1])
        if not resume:
            max_run += 1
        log_dir = f"{folder}/{run_prefix}{max_run}"
        self.log_dir = log_dir
        if tensorboard:
            self.writer = _make_writer(log_dir)
        self.cfg = get_cfg_defaults()
        self.cfg.merge_from_file(f"{folder}/config.yml")
        self.cfg.freeze()
        for k in VALID_VALUES:  # :37-39
            if self.cfg[k] not in VALID_VALUES[k]:
                raise Exception(f"Invalid value for {k}")
        for k in self.cfg:  # :41-42
            setattr(self, k, self.cfg[k])
        self.gpu_id = None
        if device is not None:  # :45-51
            self.device = torch.device(device)
            m = re.match(r".*:(\d+)", str(device))
            if m:
                self.gpu_id = int(m[1])
        else:
            self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
