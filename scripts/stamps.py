"""Dev: per-wave phase timestamps of the step kernel (QS_STAMPS=1).

python scripts/stamps.py [NAME]             one single-step launch
python scripts/stamps.py NAME --many K      one multi-step launch of K steps (QS_MAX_FUSED_STEPS=K): stamp 0 is
                                            the launch's start, stamps 1-6 are those of its last loop iteration
"""
import ctypes, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "marl-gym-pybullet-drones_amd"))
os.environ["QS_STAMPS"] = "1"
MANY = int(sys.argv[sys.argv.index("--many") + 1]) if "--many" in sys.argv else 0
if MANY:
    os.environ["QS_MAX_FUSED_STEPS"] = str(MANY)
import numpy as np, torch
from gym_pybullet_drones_amd import _lib as L
from gym_pybullet_drones_amd.envs import QuadSwarm, grid_layout
from gym_pybullet_drones_amd.utils.enums import Physics
sys.path.insert(0, ROOT)
from bench import stagger_episodes
# config: C3 (default), C5, C4 — python scripts/stamps.py [NAME]  (needs a QS_STAMPS_BUILD library)
CFG = {"C3": ("multihover", 16384, 8, "one_d_pid", Physics.DYN), "C5": ("multihover", 8192, 16, "one_d_pid", Physics.PYB_DW),
       "C4": ("spiral", 8192, 5, "vel", Physics.DYN)}[sys.argv[1] if len(sys.argv) > 1 else "C3"]
task, E, D, actn, phys = CFG
kw = dict(initial_xyzs=grid_layout(D)) if task == "multihover" else {}
sw = QuadSwarm(task, num_envs=E, num_drones=D, act=actn, precision=4, physics=phys, **kw)
obs = torch.empty((E, D, sw.obs_dim), device="cuda"); act = torch.empty((E, D, sw.act_dim), device="cuda")
sw.reset(0, obs=obs)
stagger_episodes(sw, task)
for t in range(20):
    sw.step(None, obs=obs, actions_out=act)
if MANY:
    # one set of output buffers per step: steps share a launch only while their buffers are distinct
    ring = [dict(obs=torch.empty_like(obs), actions_out=torch.empty_like(act), reward=torch.empty_like(sw.reward),
                 terminated=torch.empty_like(sw.terminated), truncated=torch.empty_like(sw.truncated))
            for _ in range(MANY)]
    for t in range(3):
        sw.step_many(ring)
torch.cuda.synchronize()
G = -(-E // (64 // D))
buf = np.zeros(G * 8, np.uint64)
lib = L.load(); lib.qs_debug_stamps.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64]
L.check(lib.qs_debug_stamps(sw._h, buf.ctypes.data_as(ctypes.c_void_p), G * 8), "stamps")
st = buf.reshape(G, 8).astype(np.float64) * 10e-3   # 100 MHz → µs
t0 = st[:, 0].min()
names = ["start", "loads used", "action/pid done", "substeps done", "reward/reset done", "obs waited", "obs stored"]
print("phase (µs, relative to first wave start): p10 / median / p90")
for k in range(7):
    v = st[:, k] - t0
    print(f"{names[k]:20s} {np.percentile(v,10):7.2f} {np.median(v):7.2f} {np.percentile(v,90):7.2f}")
d = np.diff(st[:, :7], axis=1)
print("per-wave phase durations median:", np.round(np.median(d, axis=0), 2))
if MANY:
    # the last iteration: draw (loop top -> 1) is not stamped; 1->2 PID + action stores, 2->3 substeps + readback,
    # 3->4 reward / reduction / log, 4->5 terminal obs + auto-reset, 5->6 obs span (on the fast obs path: the rows
    # into LDS only; the span's read-back brackets the draw and its stores fall into 1->2 of the next iteration)
    it = st[:, 6] - st[:, 1]
    per = (st[:, 6] - st[:, 0]) / MANY
    print("last iteration, per-wave medians (us): " + "  ".join(
        f"{names[k]}->{names[k + 1]} {np.median(d[:, k]):.3f}" for k in range(1, 6)))
    print("last iteration stamps 1->6: median %.3f us; (stamp 6 - launch start) / %d steps: median %.3f us, p90 %.3f us"
          % (np.median(it), MANY, np.median(per), np.percentile(per, 90)))
    print("launch: last wave done at %.2f us = %.3f us per step" % ((st[:, 6] - t0).max(), (st[:, 6] - t0).max() / MANY))
    sys.exit(0)
print("last wave obs stored at %.2f us; waves started by: p50 %.2f, max %.2f" % (
    (st[:, 6] - t0).max(), np.median(st[:, 0] - t0), (st[:, 0] - t0).max()))
# how many waves are in each phase over time (0.5 us bins)
bins = np.arange(0, (st[:, 6] - t0).max() + 0.5, 0.5)
for b in bins:
    ph = [(((st[:, k] - t0) <= b) & ((st[:, k + 1] - t0) > b)).sum() for k in range(6)]
    print(f"t={b:5.1f}  " + " ".join(f"{n:5d}" for n in ph))
