"""Sensors for the sensing-grid evaluator (`qr_sensing_*`, `qr_evaluate_policy_sensing_grid`, csrc/quadrace_eval_sensing.hip) and for
training under them (`qr_rollout_policy_sensing`, csrc/quadrace_rollout_sensing.hip, `PPO(sensing=...)`).

A *sensor* is what lies between the env and the policy: white Gaussian noise on the observation the policy sees, one sigma per group of
observation entries, and a command delay of 0..4 control steps (layout, stream and queue rule: include/quadrace.h).  `SensingParams`
holds one, `noise_sweep` / `delay_sweep` build the two curves a user asks for first, `SensingBank` is the device bank.  Everything but
`SensingBank` needs neither torch nor a GPU; `plan_sensor_mix` is what `PPO(sensing=...)` decides on the host."""
import ctypes as C

import numpy as np

SIGMA_FIELDS = ("sigma_pos", "sigma_vel", "sigma_att", "sigma_rate", "sigma_act", "sigma_gate_pos", "sigma_gate_yaw", "sigma_dist")
MAX_DELAY = 4
SLOT_FLOATS = 32   # a bank slot: sigma[0..7], the delay as an int32 bit pattern, zeros (128 bytes)
QUEUE_FLOATS = 4 * MAX_DELAY   # the command queue of an env: `pending` is [num_envs][16]


class SensingParams:
    """One sensor: eight sigmas, in the units of the (normalised) observation the policy sees, and `delay_steps` in [0, 4].
      sigma_pos / sigma_vel    position / velocity in the gate frame            sigma_att / sigma_rate   roll, pitch, yaw / body rates
      sigma_act                actuator state (motor speeds / T_norm)           sigma_gate_pos / _yaw    the gates ahead
      sigma_dist               the disturbance columns (E2E only; ignored by INDI)"""

    def __init__(self, name="sensor", sigma_pos=0.0, sigma_vel=0.0, sigma_att=0.0, sigma_rate=0.0, sigma_act=0.0, sigma_gate_pos=0.0,
                 sigma_gate_yaw=0.0, sigma_dist=0.0, delay_steps=0):
        sig = np.array([sigma_pos, sigma_vel, sigma_att, sigma_rate, sigma_act, sigma_gate_pos, sigma_gate_yaw, sigma_dist], dtype=np.float64)
        for field, s in zip(SIGMA_FIELDS, sig):
            if not np.isfinite(s) or s < 0.0:
                raise ValueError("%s must be finite and >= 0" % field)
        with np.errstate(over="ignore"):
            sigma = np.abs(sig.astype(np.float32))   # (-0.0 -> +0.0)
        if not np.isfinite(sigma).all():
            raise ValueError("a sigma does not fit float32")
        if int(delay_steps) != delay_steps or not 0 <= int(delay_steps) <= MAX_DELAY:
            raise ValueError("delay_steps must be an integer in [0, %d]" % MAX_DELAY)
        self.name, self.sigma, self.delay_steps = str(name), sigma, int(delay_steps)

    @classmethod
    def ideal(cls, name="ideal"):
        """No noise, no delay: the policy sees the observation of the step and its command flies in the step."""
        return cls(name)

    @classmethod
    def from_sigma(cls, sigma8, delay_steps=0, name="sensor"):
        return cls(name, *[float(s) for s in np.asarray(sigma8).reshape(8)], delay_steps=delay_steps)

    def scaled(self, factor, name=None):
        """Every sigma times `factor` (>= 0, rounded to float32 once); the delay stays."""
        f = float(factor)
        if not np.isfinite(f) or f < 0.0:
            raise ValueError("factor must be finite and >= 0")
        return SensingParams.from_sigma(self.sigma.astype(np.float64) * f, self.delay_steps, name or "%s x %g" % (self.name, f))

    def with_delay(self, d, name=None):
        return SensingParams.from_sigma(self.sigma, d, name or "%s, delay %d" % (self.name, int(d)))

    @property
    def is_ideal(self):
        return self.delay_steps == 0 and not self.sigma.any()

    def pack(self):
        """The bank slot: 32 float32 (sigma, the delay's int32 bit pattern, zeros)."""
        slot = np.zeros(SLOT_FLOATS, dtype=np.float32)
        slot[:8] = self.sigma
        slot[8:9].view(np.int32)[0] = self.delay_steps
        return slot

    @classmethod
    def unpack(cls, slot, name="sensor"):
        slot = np.ascontiguousarray(slot, dtype=np.float32).reshape(SLOT_FLOATS)
        if slot[9:].view(np.int32).any():
            raise ValueError("a sensing slot is zero behind its nine values")
        return cls.from_sigma(slot[:8], int(slot[8:9].view(np.int32)[0]), name)

    def __eq__(self, other):
        return isinstance(other, SensingParams) and self.delay_steps == other.delay_steps and \
            np.array_equal(self.sigma.view(np.int32), other.sigma.view(np.int32))

    def __repr__(self):
        return "SensingParams(%r, %s, delay_steps=%d)" % (self.name, ", ".join("%s=%g" % (f, s) for f, s in zip(SIGMA_FIELDS, self.sigma) if s),
                                                           self.delay_steps)


def noise_sweep(base, scales):
    """[base.scaled(s) for s in scales]: one sensor per noise scale, the delay of `base` in all."""
    return [base.scaled(s) for s in scales]


def delay_sweep(base, delays):
    """[base.with_delay(d) for d in delays]: one sensor per command delay, the sigmas of `base` in all."""
    return [base.with_delay(d) for d in delays]


def plan_sensor_mix(n_envs, envs_per_group, sensing, sensing_of_group=None):
    """Everything `PPO(sensing=...)` decides on the host, checked before a device is touched: (the group map, one name per bank slot).
    `sensing` is a non-empty list of SensingParams, one bank slot each; group g of `envs_per_group` envs flies through sensor
    sensing_of_group[g] (default g % S: round-robin; fewer groups than sensors is an error, as for a fixed ensemble of vehicles)."""
    n, e = int(n_envs), int(envs_per_group)
    if e < 256 or e % 256 != 0:
        raise ValueError("envs_per_group must be a multiple of 256, at least 256 (one workgroup serves one group)")
    if n < e or n % e != 0:
        raise ValueError("num_envs must be a whole number of groups of envs_per_group envs")
    groups = n // e
    if isinstance(sensing, SensingParams):
        raise ValueError("sensing must be a non-empty list of SensingParams (one sensor: [sensor])")
    sensors = list(sensing)
    if not sensors or not all(isinstance(s, SensingParams) for s in sensors):
        raise ValueError("sensing must be a non-empty list of SensingParams")
    if sensing_of_group is None:
        if groups < len(sensors):
            raise ValueError("%d groups cannot fly %d sensors: lower envs_per_group or pass fewer sensors" % (groups, len(sensors)))
        sog = [g % len(sensors) for g in range(groups)]
    else:
        sog = [int(s) for s in sensing_of_group]
    if len(sog) != groups or any(s < 0 or s >= len(sensors) for s in sog):
        raise ValueError("sensing_of_group must name one of the %d sensors for each of the %d groups" % (len(sensors), groups))
    return sog, [s.name for s in sensors]


class SensingBank:
    """`capacity` sensors side by side on the device (`qr_sensing_bank_*`): the argument of `env.evaluate_sensing_grid_device`.  A bank
    belongs to no env variant.  No CPU fallback."""

    def __init__(self, capacity, device=None):
        import torch

        from . import _lib

        self._lib = _lib
        self._L = _lib.load()
        self._h = None
        if not torch.cuda.is_available():
            raise RuntimeError("SensingBank needs a gfx950 GPU: libquadrace has no CPU fallback")
        create = _lib.require(self._L, "qr_sensing_bank_create")
        self.capacity = int(capacity)
        self.params = [None] * self.capacity   # the SensingParams of every slot set so far
        self._dev_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self._dev_index)
        h = C.c_void_p()
        _lib.check(create(self._dev_index, self.capacity, C.byref(h)))
        self._h = h

    def close(self):
        if self._h is not None:
            self._L.qr_sensing_bank_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set(self, slot, params=None):
        """Slot `slot` in [0, capacity) <- `params` (a SensingParams); None = the ideal sensor (the NULL form of qr_sensing_bank_set)."""
        if params is None:
            self._lib.check(self._L.qr_sensing_bank_set(self._h, int(slot), None, 0))
            self.params[int(slot)] = SensingParams.ideal()
            return self
        sigma = np.ascontiguousarray(params.sigma, dtype=np.float32)
        self._lib.check(self._L.qr_sensing_bank_set(self._h, int(slot), sigma.ctypes.data_as(C.POINTER(C.c_float)), int(params.delay_steps)))
        self.params[int(slot)] = params
        return self

    def read(self, slot):
        """(sigma [8] float32, delay) as slot `slot` holds them on the device."""
        sigma, delay = np.empty(8, dtype=np.float32), C.c_int32(-1)
        self._lib.check(self._L.qr_sensing_bank_read(self._h, int(slot), sigma.ctypes.data_as(C.POINTER(C.c_float)), C.byref(delay)))
        return sigma, int(delay.value)
