"""SQ counter split of the multi-step C3 step kernel (the FUSE instance), from `rocprofv3 --pmc`
passes over `scripts/pmc_probe_many.py` (each pass a run of its own, counters only, no tracing):

  rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU -d A ... -- python scripts/pmc_probe_many.py
  rocprofv3 --pmc SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_WAIT_INST_LDS SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS -d B ... -- (the same)
  python scripts/sq_report_many.py OUT.json DEPTH A B

Per 32-step launch (median over the probe's launches) and as shares of SQ_WAVE_CYCLES: issuing
VALU (SQ_ACTIVE_INST_VALU), issuing anything (SQ_ACTIVE_INST_ANY), parked on a wait count or barrier
(SQ_WAIT_ANY), issue-stalled (SQ_WAIT_INST_ANY), and the instruction counts per wave and step.
QS_DEV_LIB selects the library the probe loads."""
import csv
import glob
import json
import sys


def main(out, depth, dirs):
    acc = {}
    for d in dirs:
        for f in glob.glob(f"{d}/**/*counter_collection.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                k = r["Kernel_Name"]
                if "step_kernel<" not in k:
                    continue
                targs = k.split("step_kernel<", 1)[1].split(">", 1)[0].split(",")
                if len(targs) > 6 and targs[6].strip() == "1":
                    acc.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    med = {k: sorted(v)[len(v) // 2] for k, v in acc.items()}
    rec = {"kernel": "multi-step C3 step_kernel", "steps_per_launch": depth,
           "launches": max((len(v) for v in acc.values()), default=0), "counters_median_per_launch": med}
    wc = med.get("SQ_WAVE_CYCLES")
    if wc:
        rec["share_of_wave_cycles"] = {k: med[k] / wc for k in ("SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_ANY", "SQ_WAIT_ANY",
                                                                "SQ_WAIT_INST_ANY", "SQ_WAIT_INST_LDS") if k in med}
    waves = med.get("SQ_WAVES")
    if waves:
        rec["per_wave_and_step"] = {k: med[k] / waves / depth for k in ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_LDS",
                                                                        "SQ_WAVE_CYCLES") if k in med}
    print(json.dumps(rec, indent=1))
    json.dump(rec, open(out, "w"), indent=1)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), sys.argv[3:])
