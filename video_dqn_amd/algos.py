"""The head algorithms of the TD loss, one row each: implicit Q-learning, Gaussian distributional Q-learning, discrete BCQ.

A head algorithm is a loss launch of its own that reads one extra head behind the Q layer.  Its row says, once, what the config
checks (trainer.check_*), TDStepper, NetEngine, the model and the trainer's log lines and scalars read: its keys, its head, its
engine entries, its statistics, its held-out metrics, and why it refuses what it does not cover.  (csrc/engine.hip kAlgos: the same table on the C side.)"""
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

# the TD family's modifiers, which every head algorithm excludes: (config key, TDStepper argument, "it is on", what the head's launch lacks)
MODIFIERS = (("CQL_ALPHA", "cql_alpha", "CQL_ALPHA > 0", "has no conservative penalty"),
             ("CQL_CALIBRATED", "cql_calibrated", "CQL_CALIBRATED", "takes no Monte-Carlo return table"),
             ("MC_RETURN_FLOOR", "mc_floor", "MC_RETURN_FLOOR", "takes no Monte-Carlo return table"))


@dataclass(frozen=True)
class Algo:
    key: str                # the config key that turns it on ...
    on: Callable            # ... when on(value); never raises: what is no valid value is off here and refused by its own check
    on_text: str            # how a message says that it is on
    params: Tuple           # (config key, TDStepper argument, default) of `key` and its further keys
    head: str               # the head behind the Q layer: NetEngine(<head>_head=True), parameters <head>.weight / <head>.bias
    model_arg: str          # the HabitatDQNMultiAction argument that builds the head
    create: str             # the engine entry that creates a net with the head
    entry: str              # the engine entry of one update ...
    entry_args: Callable    # ... and its scalars, from the stepper
    stats_attr: str         # the stepper's view of loss_stats[0 : len(stats)] ...
    stats: Tuple            # ... and what its slots hold: the <name>/train scalars
    eval_entry: str         # the engine entry of one validation batch: vdqn_net_td_eval plus the head metrics launch ...
    eval_args: Callable     # ... and its scalars, from the stepper
    eval_slots: Tuple       # what the eight slots of a category's row of the head table hold (slot 0 the count): the <name>/val scalars
    title: str              # its name in log lines
    log: Callable           # stepper -> the rest of its start-up line
    word: str               # "the <word> loss launch"
    no_linear: str          # why LINEAR is refused
    min_actions: int = 1
    one_action: str = ""    # (min_actions 2) why one action column is refused
    no_loss_kind: Optional[str] = None  # why LOSS_KIND other than l2 is refused
    cql_note: str = ""      # what its refusal of CQL_ALPHA adds
    eval_sample_slots: Tuple = ()  # what the slots of the head table's per-sample row hold (slot 0 the count); (): the row stays zero

    @property
    def head_keys(self):
        return (f"{self.head}.weight", f"{self.head}.bias")

    def is_on(self, config) -> bool:
        return self.on(getattr(config, self.key, self.params[0][2]))

    def kwargs(self, config) -> dict:
        """TDStepper's arguments of this algorithm from the config (None: the default)."""
        got = ((arg, default, getattr(config, key, default)) for key, arg, default in self.params)
        return {arg: type(default)(default if v is None else v) for arg, default, v in got}


ALGOS = (
    Algo(key="IQL_EXPECTILE", on=lambda v: isinstance(v, (int, float)) and v > 0, on_text="IQL_EXPECTILE > 0",
         params=(("IQL_EXPECTILE", "iql_expectile", 0.0),),
         head="value", model_arg="value_head", create="vdqn_net_create_v",
         entry="vdqn_net_td_forward_iql", entry_args=lambda s: (s.iql_expectile,),
         stats_attr="iql_stats", stats=("iql_v_loss", "iql_advantage"),  # the V loss alone, the mean advantage of the data action
         eval_entry="vdqn_net_td_eval_iql", eval_args=lambda s: (s.iql_expectile,),
         # the expectile loss, Q_target(s, a_data) - V(s), the loss and |error| of Q(s, a_data) against r + GAMMA (1 - t) V(s'), V(s),
         # that target, the share of positive advantages
         eval_slots=("count", "iql_v_loss", "iql_advantage", "iql_q_loss", "iql_td_abs_error", "iql_value", "iql_td_target",
                     "iql_positive_share"),
         title="implicit Q-learning",
         log=lambda s: f"a value head V(s) fitted to Q_target(s, a_data) at expectile {s.iql_expectile:g}, Q(s, a_data) regressed on "
                       "r + GAMMA (1 - t) V(s') in the loss launch; the target pass runs over s",
         word="IQL", no_linear="y = r + (Qa - 0.1) is the undiscounted Double-DQN target and has no V(s') form",
         min_actions=2, one_action="whose Q(s, a) is the state value already",
         cql_note=" (implicit Q-learning avoids out-of-data actions instead of penalising them)"),
    Algo(key="DISTRIBUTIONAL", on=lambda v: v is True, on_text="DISTRIBUTIONAL",
         params=(("DISTRIBUTIONAL", "distributional", False), ("KL_BACKWARDS", "kl_backwards", False), ("LOG_SIGMA", "log_sigma", False),
                 ("DIST_SIGMA_MIN", "sigma_min", 0.1)),
         head="spread", model_arg="distributional", create="vdqn_net_create_d",
         entry="vdqn_net_td_forward_dist", entry_args=lambda s: (s.dist_flags, s.sigma_min),
         stats_attr="dist_stats", stats=("dist_sigma", "dist_z2"),  # mean predicted sigma at the data action, mean squared standardised error
         eval_entry="vdqn_net_td_eval_dist", eval_args=lambda s: (s.dist_flags, s.sigma_min),
         # the KL, the predicted sigma, the squared standardised error, the Gaussian NLL of the backup's mean (constant dropped), the
         # one-sigma coverage (0.683 when calibrated), the backup's sigma, the predicted sigma of the greedy action
         eval_slots=("count", "dist_kl", "dist_sigma", "dist_z2", "dist_nll", "dist_coverage", "dist_backup_sigma", "dist_greedy_sigma"),
         title="distributional Q-learning",
         log=lambda s: "a Gaussian over the return per (category, action), a spread head behind the Q layer; the loss is KL("
                       + ("prediction || backup" if s.dist_flags & 1 else "backup || prediction") + ") against the Double-DQN backup's Gaussian, sigma "
                       + ("= exp(rho)" if s.dist_flags & 2 else "= softplus(rho)") + f" with the floor {s.sigma_min:g}",
         word="distributional", no_linear="y = r + (Qa - 0.1) has no discount to back a variance up with",
         no_loss_kind="the loss is a KL divergence between two Gaussians, which has no Huber form"),
    Algo(key="BCQ_THRESHOLD", on=lambda v: isinstance(v, (int, float)) and v >= 0, on_text="BCQ_THRESHOLD",
         params=(("BCQ_THRESHOLD", "bcq_threshold", -1.0), ("BCQ_BC_WEIGHT", "bcq_bc_weight", 1.0), ("BCQ_LOGIT_REG", "bcq_logit_reg", 0.01)),
         head="policy", model_arg="policy_head", create="vdqn_net_create_p",
         entry="vdqn_net_td_forward_bcq", entry_args=lambda s: (s.bcq_threshold, s.bcq_bc_weight, s.bcq_logit_reg),
         stats_attr="bcq_stats", stats=("bcq_bc_loss", "bcq_constrained_share", "bcq_accuracy"),  # (share: of targets the constraint changed)
         eval_entry="vdqn_net_td_eval_bcq", eval_args=lambda s: (s.bcq_threshold,),
         # the loss and |error| against the constrained target, that target, the share of targets the constraint changes, the agreement
         # of the constrained policy at s with the data, the share of states where the constraint changes the greedy action, its Q
         eval_slots=("count", "bcq_q_loss", "bcq_td_abs_error", "bcq_td_target", "bcq_constrained_share", "bcq_policy_agreement",
                     "bcq_policy_changed", "bcq_q_policy"),
         # per sample: the cross-entropy, the behaviour accuracy, mean_a i_a^2, the allowed actions at s, pi_b(a_data), the allowed at s'
         eval_sample_slots=("samples", "bcq_bc_loss", "bcq_accuracy", "bcq_logit_sq", "bcq_allowed_actions", "bcq_data_prob",
                            "bcq_allowed_actions_next"),
         title="batch-constrained Q-learning",
         log=lambda s: f"a policy head behind the Q layer fitted to the logged actions (weight {s.bcq_bc_weight:g}, "
                       f"logit regulariser {s.bcq_logit_reg:g}); the target's arg-max at s' runs over the actions with pi_b / max pi_b > "
                       f"{s.bcq_threshold:g} under the online head",
         word="BCQ", no_linear="the constrained target is not defined for y = r + (Qa - 0.1)",
         min_actions=2, one_action="and with one action there is nothing to constrain"),
)
IQL, DIST, BCQ = ALGOS
HEAD_EVAL_SLOTS = 8  # of a row of the head table, f64 [num_classes + 1][8] (csrc/eval.hip)
LOSS_SLOTS = 4  # of TDStepper.loss_stats: the TD family's cql_penalty and mc_stats side by side, or a head algorithm's statistics


def refuse(algo: Algo, config, say=str, error=ValueError, prefix="") -> None:
    """While `algo` is on: raise `error` for the first thing about `config` that it does not cover.  `config` has the config's keys;
    say(key) is the name a message gives a key (TDStepper: its argument of that meaning)."""
    def get(key):
        return getattr(config, key, False)

    def no(text):
        raise error(f"{prefix}{say(algo.key)} {text}")
    if not algo.is_on(config):
        return
    if get("TRAIN_ON_GROUND_TRUTH"):
        no(f"needs the TD branch: {say('TRAIN_ON_GROUND_TRUTH')} regresses Q(s, a) on given targets and bootstraps nothing")
    if get("LINEAR"):
        no(f"does not cover {say('LINEAR')}: {algo.no_linear}")
    for key in ("VALUE_LEARNING", "ONE_ACTION"):
        if algo.min_actions > 1 and get(key):
            no(f"needs more than one action: {say(key)} builds a network with one action column, {algo.one_action}")
    if algo.no_loss_kind and str(getattr(config, "LOSS_KIND", "l2")) != "l2":
        no(f"with {say('LOSS_KIND')}: {config.LOSS_KIND} — {algo.no_loss_kind}")
    for key, _, on_text, lacks in MODIFIERS:
        if float(get(key)) > 0:
            no(f"with {on_text.replace(key, say(key))} is deliberately out of scope: the {algo.word} loss launch {lacks}"
               f"{algo.cql_note if key == 'CQL_ALPHA' else ''}; use one or the other")
    for other in ALGOS:
        if other is not algo and other.is_on(config):  # one text per pair, whichever row's check meets it: the later row's key first
            a, b = sorted((algo, other), key=ALGOS.index)
            raise error(f"{prefix}{say(b.key)} with {a.on_text.replace(a.key, say(a.key))} is deliberately out of scope: one extra head "
                        f"sits behind the Q layer, the {a.head} head or the {b.head} head; use one or the other")


def eval_tags(algo: Algo) -> Tuple:
    """((scalar tag, key of eval_result()["head"]), ..) of `algo`'s held-out metrics: <slot name>/val, the counts left out."""
    return tuple((f"{name}/val", name) for name in algo.eval_slots[1:] + algo.eval_sample_slots[1:])
