"""HBM traffic of the C3 step kernel, one step per launch against several (qs_step_many).

Probe (under `rocprofv3 --pmc FETCH_SIZE -- python scripts/pmc_probe_many.py`, then the
same with WRITE_SIZE, each pass a run of its own with no tracing): a known-byte
calibration copy (scripts/pmc_probe.py's), ten single steps, then 64 random-policy steps
through `step_many` — launches of QS_MAX_FUSED_STEPS steps — or, on a build without
it, 64 single steps.

Report (`python scripts/pmc_probe_many.py report FETCH_DIR WRITE_DIR DEPTH`): calibrated
bytes per launch of the single-step and of the multi-step kernel (told apart by the
FUSE template argument in the kernel name), and per agent-step (÷ agents · DEPTH for the latter).
QS_PKG_DIR points the probe at another tree's package directory."""
import csv
import ctypes
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CAL = 1 << 26   # 256 MiB each way
E, D, STEPS = 16384, 8, 64


def probe():
    sys.path.insert(0, os.environ.get("QS_PKG_DIR", os.path.join(ROOT, "marl-gym-pybullet-drones_amd")))
    import torch
    from gym_pybullet_drones_amd import _lib as L
    from gym_pybullet_drones_amd.envs import QuadSwarm, grid_layout
    torch.cuda.set_device(0)
    lib = L.load()
    src = torch.rand(N_CAL, device="cuda")
    dst = torch.empty_like(src)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(3):
        L.check(lib.qs_calib_copy(L.ptr(dst), L.ptr(src), N_CAL, st), "calib")
    sw = QuadSwarm("multihover", num_envs=E, num_drones=D, act="one_d_pid", initial_xyzs=grid_layout(D))
    slots = 32
    obs = torch.empty((slots, E, D, sw.obs_dim), device="cuda")
    act = torch.empty((slots, E, D, sw.act_dim), device="cuda")
    rew = torch.empty((slots, E), dtype=sw.reward.dtype, device="cuda")
    te = torch.empty((slots, E), dtype=torch.uint8, device="cuda")
    tr = torch.empty((slots, E), dtype=torch.uint8, device="cuda")
    kw = lambda t: dict(obs=obs[t % slots], reward=rew[t % slots], terminated=te[t % slots],
                        truncated=tr[t % slots], actions_out=act[t % slots])
    sw.reset(0, obs=obs[0])
    for t in range(10):
        sw.step(None, **kw(t))
    if hasattr(sw, "step_many"):
        sw.step_many([kw(t) for t in range(STEPS)])
    else:
        for t in range(STEPS):
            sw.step(None, **kw(t))
    torch.cuda.synchronize()
    print("calib bytes each way", N_CAL * 4, "agents", E * D, "steps", STEPS)


def per_kernel(d, counter):
    acc = {}
    for f in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if r.get("Counter_Name") == counter:
                acc.setdefault(r["Kernel_Name"], []).append(float(r["Counter_Value"]))
    return acc


def report(fetch_dir, write_dir, depth):
    f, w = per_kernel(fetch_dir, "FETCH_SIZE"), per_kernel(write_dir, "WRITE_SIZE")
    cal = [k for k in f if "calib_copy" in k][0]
    cf = N_CAL * 4 / (sum(f[cal]) / len(f[cal]) * 1024)
    cw = N_CAL * 4 / (sum(w[cal]) / len(w[cal]) * 1024)
    med = lambda v: sorted(v)[len(v) // 2]
    out = {"fetch_scale": cf, "write_scale": cw, "workload": {"envs": E, "drones": D, "act": "one_d_pid"}, "kernels": {}}
    for k in f:
        if "step_kernel" not in k:
            continue
        targs = k.split("step_kernel<", 1)[1].split(">", 1)[0].split(",")   # <T, TASK, ACT, CF, PHYS, AUXM[, FUSE]>
        many = len(targs) > 6 and targs[6].strip() == "1"
        steps = depth if many else 1
        fb, wb = med(f[k]) * 1024 * cf, med(w[k]) * 1024 * cw
        out["kernels"]["multi_step" if many else "single_step"] = {
            "kernel": k, "launches": len(f[k]), "steps_per_launch": steps, "fetch_bytes_per_launch": fb,
            "write_bytes_per_launch": wb, "traffic_per_agent_step": (fb + wb) / (E * D * steps)}
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "report":
        report(sys.argv[2], sys.argv[3], int(sys.argv[4]))
    else:
        probe()
