#!/usr/bin/env python
"""ms per micro-batch of Stage 2's three training modes at one config's shapes (default cfg4: bs 16, 575 + 64 + 256
tokens), synthetic weights and data as bench.py's Stage-2 run:

  A  LLM trained, projector frozen (bench.py --config cfg4)     B  LLM and projector trained
  C  LLM frozen, projector trained

    python tools/stage2_modes_bench.py [--modes A,B,C] [--steps 3] [--warmup 1] [--gas 8] [--out FILE.json]

Each mode runs in a fresh child process (one engine on the device at a time); inside it the warm-up and the timed
steps each run under their own time limit (a watchdog ends the process with status 124 when a phase overruns), and
the parent starts the next mode only after a child that ended well.  After the timed steps, --stage-steps more
steps run with the stage timers on: the `projector.bwd` stage's ms per micro-batch is reported next to the total.
One JSON line per mode on stdout."""
import argparse
import json
import os
import subprocess
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = {"A": (True, False), "B": (True, True), "C": (False, True)}


class Phase:
    """`with Phase("warm-up", seconds):` -- the process ends (124) if the block runs longer."""

    def __init__(self, name, seconds):
        self.t = threading.Timer(seconds, self.expired, (name, seconds))
        self.t.daemon = True

    @staticmethod
    def expired(name, seconds):
        sys.stderr.write(f"stage2_modes_bench: {name} exceeded its {seconds} s limit\n")
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.t.start()

    def __exit__(self, *exc):
        self.t.cancel()
        return False


def child(a):
    import torch
    from projectiontrainer_amd import _lib as L
    from projectiontrainer_amd import weights as W
    from projectiontrainer_amd.config import PRESETS
    from projectiontrainer_amd.stage2 import synthetic_engine
    cfg = PRESETS[a.config]
    dev = torch.device("cuda:0")
    train_llm, train_projector = MODES[a.mode]
    eng = synthetic_engine(cfg, dev, seed=0, total_steps=10 ** 6, gradient_accumulation_steps=a.gas,
                           learning_rate=1e-5, train_llm=train_llm, train_projector=train_projector)
    px, q, ans = (torch.from_numpy(t).to(dev) for t in W.synthetic_vqa_batch(cfg, seed=1234))

    def step():
        for _ in range(a.gas):
            loss = eng.forward_backward(px, q, ans)
        eng.optimizer_step()
        return loss

    with Phase("warm-up", a.warmup_limit):
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
    with Phase("timed steps", a.steps_limit):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(a.steps):
            loss = step()
        ev[1].record()
        torch.cuda.synchronize()
        ms = ev[0].elapsed_time(ev[1]) / (a.steps * a.gas)
    stages = {}
    if a.stage_steps:
        with Phase("stage-timer steps", a.steps_limit):
            L.stage_timers_enable(True)
            L.stage_timers_read(reset=True)
            for _ in range(a.stage_steps):
                step()
            torch.cuda.synchronize()
            L.stage_timers_enable(False)
            n = a.stage_steps * a.gas
            stages = {k: round(v[0] / n, 4) for k, v in L.stage_timers_read(reset=True).items()
                      if k in ("projector.fwd", "projector.bwd", "siglip.fwd")}
    print(json.dumps({"mode": a.mode, "config": a.config, "train_llm": train_llm, "train_projector": train_projector,
                      "batch": cfg.batch_size, "seq_len": cfg.seq_len, "gas": a.gas, "steps": a.steps,
                      "ms_per_micro_batch": round(ms, 3), "images_per_s": round(cfg.batch_size / ms * 1e3, 2),
                      "stage_ms_per_micro_batch": stages, "loss": round(float(loss), 5)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="A,B,C")
    ap.add_argument("--mode", default=None, help="(child) the one mode to run")
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--stage-steps", type=int, default=1)
    ap.add_argument("--gas", type=int, default=8)
    ap.add_argument("--warmup-limit", type=float, default=120.0, help="seconds for the warm-up steps")
    ap.add_argument("--steps-limit", type=float, default=120.0, help="seconds for the timed steps")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode is not None:
        return child(a)
    lines = []
    for m in a.modes.split(","):
        argv = [sys.executable, os.path.abspath(__file__), "--mode", m] + [x for x in sys.argv[1:]]
        # the child's own phase limits end it first; this bound covers its start-up (weights, first launches)
        r = subprocess.run(argv, stdout=subprocess.PIPE, text=True,
                           timeout=a.warmup_limit + 2 * a.steps_limit + 180)
        if r.returncode != 0:
            sys.exit(f"mode {m} ended with status {r.returncode}: nothing more is started on the device")
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
