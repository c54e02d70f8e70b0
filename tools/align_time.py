"""Dev tool: time lasr_ctc_align against lasr_ctc_loss with grad = NULL (the lattice launch alone) in the same process, at the
bench shape cfg2 (B=32, T'=501, C=28, S~150), cfg5 (C=4334) and the dev envelope (B=2, T'=2001, S=600).  Events around `reps`
replays after warm-up, workspaces and outputs allocated once.  Writes profiles/ctc_align_time.json.
python tools/align_time.py [reps]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from lightning_asr_amd import _lib, ops  # noqa: E402

SHAPES = {"cfg2": (32, 501, 28, 150), "cfg5": (32, 501, 4334, 150), "dev_envelope": (2, 2001, 28, 600)}


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
    dev = torch.device("cuda")
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    out = {"reps": reps, "unit": "us per call", "shapes": {}}
    for name, (B, T, C, S) in SHAPES.items():
        g = torch.Generator().manual_seed(1)
        logp = torch.randn(B, T, C, generator=g).log_softmax(-1).to(dev).contiguous()
        tl_h = torch.randint(max(S - S // 4, 1), S + 1, (B,), generator=g).to(torch.int32)
        tl_h[0] = S
        tg = torch.randint(0, C - 1, (B, S), generator=g).to(dev)
        il = torch.full((B,), T, dtype=torch.int32, device=dev)
        tl = tl_h.to(dev)
        nll = torch.empty(B, device=dev)
        nb_loss = int(lib.lasr_ctc_workspace_bytes(B, T, S))
        ws_loss = torch.empty(nb_loss, dtype=torch.uint8, device=dev)
        al = ops.ctc_align(logp, tg, il, tl, C - 1)                     # outputs reused below
        nb_al = int(lib.lasr_ctc_align_workspace_bytes(B, T, S))
        ws_al = torch.empty(nb_al, dtype=torch.uint8, device=dev)

        def loss():
            _lib.call("lasr_ctc_loss", logp.data_ptr(), tg.data_ptr(), il.data_ptr(), tl.data_ptr(), B, T, C, S, C - 1, nll.data_ptr(), None,
                      None, ws_loss.data_ptr(), nb_loss, st)

        def align():
            _lib.call("lasr_ctc_align", logp.data_ptr(), tg.data_ptr(), il.data_ptr(), tl.data_ptr(), B, T, C, S, C - 1, al.score.data_ptr(),
                      al.frame_state.data_ptr(), al.frame_logp.data_ptr(), al.label_start.data_ptr(), al.label_end.data_ptr(),
                      ws_al.data_ptr(), nb_al, st)

        t_loss, t_align = timed(loss, reps), timed(align, reps)
        torch.cuda.synchronize()
        assert bool((al.score <= -nll + 1e-4 * nll.abs().clamp(min=1)).all())
        out["shapes"][name] = {"B": B, "T": T, "C": C, "S": S, "ctc_loss_lattice_us": round(t_loss, 1), "ctc_align_us": round(t_align, 1),
                               "workspace_bytes": {"ctc_loss": nb_loss, "ctc_align": nb_al}}
        print("%-13s B=%d T'=%d C=%d S=%d: lasr_ctc_loss(grad=NULL) %.1f us, lasr_ctc_align %.1f us" % (name, B, T, C, S, t_loss, t_align))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    os.makedirs(os.path.join(root, "profiles"), exist_ok=True)
    with open(os.path.join(root, "profiles", "ctc_align_time.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
