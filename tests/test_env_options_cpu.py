"""The env's option table (env.ENV_OPTIONS) as every Python layer reads it:
the trainer's config and command line cover it, the refusals of DroneBatch
and PPOConfig are the ones recorded before the table existed (type and full
text, and which one comes first where an input breaks two rules), and the
vector envs pass the keywords through.  No device: every refusal here comes
before any device work.
"""
import dataclasses

import pytest

from drone_rl_amd import train
from drone_rl_amd.env import (ENV_OPTION_KEYS, ENV_OPTIONS, EXCLUSIONS, DroneBatch,
                              check_env_options, option_values)
from drone_rl_amd.ppo import PPOConfig
from drone_rl_amd.vec_env import BatchedDroneVecEnv, DroneVectorEnv

nan, inf = float("nan"), float("inf")
DEFAULTS = {k: d for o in ENV_OPTIONS for k, d in zip(o.keys, o.defaults)}


# ---------------------------------------------------------------- coverage
def test_table_shape():
    assert [o.name for o in ENV_OPTIONS] == ["smoothing", "tag", "wind", "waypoints", "airframe"]
    assert [o.field for o in ENV_OPTIONS] == [None, None, "wind", "waypoint", "airframe"]
    assert len(ENV_OPTION_KEYS) == 13 == len(set(ENV_OPTION_KEYS))
    for o in ENV_OPTIONS:
        assert len(o.keys) == len(o.defaults) == len(o.idle) == len(o.help)
        assert callable(getattr(DroneBatch, o.setter))
    names = {o.name for o in ENV_OPTIONS}
    assert all(pair <= names and len(pair) == 2 for pair in EXCLUSIONS)


def test_config_fields_cover_the_table():
    fields = {f.name: f.default for f in dataclasses.fields(PPOConfig)}
    for k in ENV_OPTION_KEYS:
        assert k in fields and fields[k] == DEFAULTS[k] and type(fields[k]) is type(DEFAULTS[k])
    assert PPOConfig().env_options() == DEFAULTS
    # old checkpoints and sb3_zip read the keys from the config's dict
    assert set(ENV_OPTION_KEYS) <= set(dataclasses.asdict(PPOConfig()))


def test_command_line_covers_the_table():
    ap = train.build_parser()
    dests = {a.dest for a in ap._actions}
    assert set(ENV_OPTION_KEYS) <= dests
    values = option_values(ap.parse_args([]))
    assert list(values) == list(ENV_OPTION_KEYS)
    assert PPOConfig(**values).env_options() == DEFAULTS
    a = ap.parse_args(["--variant", "smooth", "--motor-alpha", "0.5", "--rate-penalty", "0.01"])
    assert option_values(a) == {**DEFAULTS, "motor_alpha": 0.5, "rate_penalty": 0.01}


def test_checked_values():
    off = dict.fromkeys((o.name for o in ENV_OPTIONS))
    assert check_env_options("gym", {}) == off
    assert check_env_options("rk4", {}) == off
    assert check_env_options("smooth", {"motor_alpha": 0.5}) == {**off, "smoothing": (0.5, 0.0)}
    assert check_env_options("tag", {}, num_envs=4) == {**off, "tag": (0.25, 0.0)}
    assert check_env_options("gym", {"drag": 0.5}) == {**off, "wind": (0.5, 0.0, 0.0, 0.0)}
    assert check_env_options("gym", {"reach_bonus": 2.0}) == {**off, "waypoints": (0.25, 2.0)}
    assert check_env_options("gym", {"motor_spread": 0.5}) == {**off, "airframe": (0.0, 0.0, 0.5)}


# --------------------------------------------------------- golden refusals
# (variant, option keywords, num_envs / max_steps / env_id_offset where they
# matter, DroneBatch's refusal, PPOConfig's refusal or None where the config
# has no such setting), recorded from the constructors as they were with the
# checks written out by hand in each of them
V = "ValueError"
EVEN = "variant='tag' pairs env 2j with env 2j+1: num_envs and env_id_offset must be even, got "
NEED_WIND = "drag / wind_speed / gust_sigma / gust_rate need variant='gym', not "
NEED_AIRFRAME = "mass_spread / inertia_spread / motor_spread need variant='gym', not "
GOLDEN = [
    # check_smoothing
    ("gym", {"motor_alpha": 0.0}, {},
     (V, "motor_alpha must be in (0, 1], got 0.0"), (V, "motor_alpha must be in (0, 1], got 0.0")),
    ("smooth", {"motor_alpha": 1.5}, {},
     (V, "motor_alpha must be in (0, 1], got 1.5"), (V, "motor_alpha must be in (0, 1], got 1.5")),
    ("smooth", {"motor_alpha": nan}, {},
     (V, "motor_alpha must be in (0, 1], got nan"), (V, "motor_alpha must be in (0, 1], got nan")),
    ("smooth", {"rate_penalty": -1.0}, {},
     (V, "rate_penalty must be finite and >= 0, got -1.0"),
     (V, "rate_penalty must be finite and >= 0, got -1.0")),
    ("smooth", {"rate_penalty": inf}, {},
     (V, "rate_penalty must be finite and >= 0, got inf"),
     (V, "rate_penalty must be finite and >= 0, got inf")),
    ("gym", {"motor_alpha": 0.5}, {},
     (V, "motor_alpha / rate_penalty need variant='smooth', not 'gym'"),
     (V, "motor_alpha / rate_penalty need variant='smooth', not 'gym'")),
    ("tag", {"rate_penalty": 0.1}, {},
     (V, "motor_alpha / rate_penalty need variant='smooth', not 'tag'"),
     (V, "motor_alpha / rate_penalty need variant='smooth', not 'tag'")),
    # check_tag
    ("tag", {"tag_radius": 0.0}, {},
     (V, "tag_radius must be finite and > 0, got 0.0"),
     (V, "tag_radius must be finite and > 0, got 0.0")),
    ("tag", {"tag_radius": inf}, {},
     (V, "tag_radius must be finite and > 0, got inf"),
     (V, "tag_radius must be finite and > 0, got inf")),
    ("tag", {"crash_penalty": -1.0}, {},
     (V, "crash_penalty must be finite and >= 0, got -1.0"),
     (V, "crash_penalty must be finite and >= 0, got -1.0")),
    ("tag", {}, {"num_envs": 3}, (V, EVEN + "3 and 0"), (V, EVEN + "3 and 0")),
    ("tag", {}, {"env_id_offset": 1}, (V, EVEN + "4 and 1"), None),
    ("gym", {"tag_radius": 0.3}, {},
     (V, "tag_radius / crash_penalty need variant='tag', not 'gym'"),
     (V, "tag_radius / crash_penalty need variant='tag', not 'gym'")),
    ("smooth", {"crash_penalty": 1.0}, {},
     (V, "tag_radius / crash_penalty need variant='tag', not 'smooth'"),
     (V, "tag_radius / crash_penalty need variant='tag', not 'smooth'")),
    # check_wind
    ("gym", {"drag": -0.1}, {},
     (V, "drag must be finite and >= 0, got -0.1"), (V, "drag must be finite and >= 0, got -0.1")),
    ("gym", {"wind_speed": inf}, {},
     (V, "wind_speed must be finite and >= 0, got inf"),
     (V, "wind_speed must be finite and >= 0, got inf")),
    ("gym", {"gust_sigma": nan}, {},
     (V, "gust_sigma must be finite and >= 0, got nan"),
     (V, "gust_sigma must be finite and >= 0, got nan")),
    ("gym", {"gust_rate": 1.5}, {},
     (V, "gust_rate must be in [0, 1], got 1.5"), (V, "gust_rate must be in [0, 1], got 1.5")),
    ("gym", {"gust_rate": -0.5}, {},
     (V, "gust_rate must be finite and >= 0, got -0.5"),
     (V, "gust_rate must be finite and >= 0, got -0.5")),
    ("gym", {"drag": 60.0}, {},
     (V, "drag * dt must be <= 1 (dt = 0.02), got drag = 60.0"),
     (V, "drag * dt must be <= 1 (dt = 0.02), got drag = 60.0")),
    ("gym", {"drag": 1e39}, {},
     (V, "drag must be finite and >= 0, got 1e+39"),
     (V, "drag must be finite and >= 0, got 1e+39")),
    ("rk4", {"drag": 0.1}, {}, (V, NEED_WIND + "'rk4'"), (V, NEED_WIND + "'rk4'")),
    ("gym", {"wind_speed": 1.0}, {"max_steps": 1 << 24},
     (V, "wind needs max_steps below 2^24"), None),
    # check_waypoints
    ("gym", {"reach_radius": 0.0}, {},
     (V, "reach_radius must be finite and > 0, got 0.0"),
     (V, "reach_radius must be finite and > 0, got 0.0")),
    ("gym", {"reach_radius": -1.0}, {},
     (V, "reach_radius must be finite and > 0, got -1.0"),
     (V, "reach_radius must be finite and > 0, got -1.0")),
    ("gym", {"reach_bonus": -1.0}, {},
     (V, "reach_bonus must be finite and >= 0, got -1.0"),
     (V, "reach_bonus must be finite and >= 0, got -1.0")),
    ("gym", {"reach_bonus": inf}, {},
     (V, "reach_bonus must be finite and >= 0, got inf"),
     (V, "reach_bonus must be finite and >= 0, got inf")),
    ("moving", {"reach_radius": 0.3}, {},
     (V, "reach_radius / reach_bonus need variant='gym', not 'moving'"),
     (V, "reach_radius / reach_bonus need variant='gym', not 'moving'")),
    ("gym", {"reach_bonus": 1.0}, {"max_steps": 1 << 24},
     (V, "waypoint courses need max_steps below 2^24"), None),
    # check_airframe
    ("gym", {"mass_spread": 1.0}, {},
     (V, "mass_spread must be in [0, 0.9], got 1.0"),
     (V, "mass_spread must be in [0, 0.9], got 1.0")),
    ("gym", {"inertia_spread": -0.1}, {},
     (V, "inertia_spread must be in [0, 0.9], got -0.1"),
     (V, "inertia_spread must be in [0, 0.9], got -0.1")),
    ("gym", {"motor_spread": nan}, {},
     (V, "motor_spread must be in [0, 0.9], got nan"),
     (V, "motor_spread must be in [0, 0.9], got nan")),
    ("smooth", {"mass_spread": 0.1}, {},
     (V, NEED_AIRFRAME + "'smooth'"), (V, NEED_AIRFRAME + "'smooth'")),
    # the three exclusions
    ("gym", {"drag": 0.1, "reach_radius": 0.3}, {},
     (V, "a gym env has wind or a waypoint course, not both"),
     (V, "a gym env has wind or a waypoint course, not both")),
    ("gym", {"wind_speed": 1.0, "mass_spread": 0.1}, {},
     (V, "a gym env has wind or randomised airframes, not both"),
     (V, "a gym env has wind or randomised airframes, not both")),
    ("gym", {"reach_bonus": 1.0, "motor_spread": 0.1}, {},
     (V, "a gym env has a waypoint course or randomised airframes, not both"),
     (V, "a gym env has a waypoint course or randomised airframes, not both")),
    # two rules broken at once: which refusal comes first.  DroneBatch asks
    # the tag rules last, PPOConfig right after the smoothing rules
    ("gym", {"tag_radius": 1.0, "drag": -1.0}, {},
     (V, "drag must be finite and >= 0, got -1.0"),
     (V, "tag_radius / crash_penalty need variant='tag', not 'gym'")),
    ("gym", {"motor_alpha": 0.5, "tag_radius": 1.0}, {},
     (V, "motor_alpha / rate_penalty need variant='smooth', not 'gym'"),
     (V, "motor_alpha / rate_penalty need variant='smooth', not 'gym'")),
    ("gym", {"drag": -1.0, "reach_radius": 0.0}, {},
     (V, "drag must be finite and >= 0, got -1.0"), (V, "drag must be finite and >= 0, got -1.0")),
    ("gym", {"reach_radius": 0.0, "mass_spread": 2.0}, {},
     (V, "reach_radius must be finite and > 0, got 0.0"),
     (V, "reach_radius must be finite and > 0, got 0.0")),
    ("gym", {"mass_spread": 2.0, "crash_penalty": 1.0}, {},
     (V, "mass_spread must be in [0, 0.9], got 2.0"),
     (V, "tag_radius / crash_penalty need variant='tag', not 'gym'")),
    ("smooth", {"rate_penalty": -1.0, "drag": 0.1}, {},
     (V, "rate_penalty must be finite and >= 0, got -1.0"),
     (V, "rate_penalty must be finite and >= 0, got -1.0")),
    ("gym", {"drag": 0.1, "reach_radius": 0.3, "mass_spread": 0.1}, {},
     (V, "a gym env has wind or a waypoint course, not both"),
     (V, "a gym env has wind or a waypoint course, not both")),
    ("tag", {"drag": 0.1}, {"num_envs": 3}, (V, NEED_WIND + "'tag'"), (V, EVEN + "3 and 0")),
    ("gym", {"motor_alpha": 0.0, "rate_penalty": -1.0}, {},
     (V, "motor_alpha must be in (0, 1], got 0.0"), (V, "motor_alpha must be in (0, 1], got 0.0")),
    ("moving", {"reach_radius": 0.0}, {},
     (V, "reach_radius must be finite and > 0, got 0.0"),
     (V, "reach_radius must be finite and > 0, got 0.0")),
    ("gym", {"gust_rate": 2.0, "drag": 60.0}, {},
     (V, "gust_rate must be in [0, 1], got 2.0"), (V, "gust_rate must be in [0, 1], got 2.0")),
    ("rk4", {"inertia_spread": 0.1, "wind_speed": 1.0}, {},
     (V, NEED_WIND + "'rk4'"), (V, NEED_WIND + "'rk4'")),
    # the variant itself comes before every option
    ("nope", {"drag": -1.0}, {}, (V, "unknown variant 'nope'"), (V, "unknown variant 'nope'")),
]


def _refusal(call):
    try:
        call()
    except Exception as e:  # noqa: BLE001 - the type is what is compared
        return type(e).__name__, str(e)
    return None


@pytest.mark.parametrize("case", range(len(GOLDEN)))
def test_golden_refusal(case):
    variant, options, extra, batch, config = GOLDEN[case]
    extra = dict(extra)
    n = extra.pop("num_envs", 4)
    assert _refusal(lambda: DroneBatch(n, variant, **extra, **options)) == batch
    if config is not None:
        assert _refusal(lambda: PPOConfig(num_envs=n, variant=variant, **options)) == config


def test_the_two_orders_differ():
    """Why check_env_options keeps `last`: inputs exist that the two
    constructors have always refused with different words."""
    assert sum(1 for *_, b, c in GOLDEN if c is not None and b != c) >= 3


# ------------------------------------------------------------ pass-through
@pytest.mark.parametrize("make", [lambda **kw: DroneBatch(4, **kw),
                                  lambda **kw: BatchedDroneVecEnv(4, **kw),
                                  lambda **kw: DroneVectorEnv(4, **kw)])
def test_option_keywords_pass_through(make):
    with pytest.raises(TypeError) as e:
        make(not_an_option=1)
    assert str(e.value) == ("DroneBatch.__init__() got an unexpected keyword argument "
                            "'not_an_option'")
    # the valid spelling reaches the option's check
    with pytest.raises(ValueError) as e:
        make(gust_rate=1.5)
    assert str(e.value) == "gust_rate must be in [0, 1], got 1.5"
    with pytest.raises(ValueError) as e:
        make(variant="smooth", motor_alpha=2.0)
    assert str(e.value) == "motor_alpha must be in (0, 1], got 2.0"


def test_unknown_keyword_message_is_pythons():
    def f(a=0):
        pass
    with pytest.raises(TypeError) as e:
        f(not_an_option=1)
    want = str(e.value).replace(f.__qualname__, "DroneBatch.__init__")
    assert _refusal(lambda: DroneBatch(4, not_an_option=1)) == ("TypeError", want)
