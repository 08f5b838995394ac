"""Worker of tests/test_hip_probe_model.py: ONE rank of a `--trainer LinearProbe` runner job.  Calls ovmr_amd.cli.main with the command line
it is given and saves what the rank returned and printed, with the probe the rank fitted:

    RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT (/ LOCAL_RANK, OVMR_DIST_BACKEND, OVMR_DIST_TIMEOUT) in the environment
    argv: <result path> <runner arguments ...>      ->      <result path> = torch.save({"results", "stdout", "W", "b"})

(The decode workers of the pipelined loader re-import this file as __mp_main__: nothing heavy at module level.)"""
import io
import os
import sys
from contextlib import redirect_stdout

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from ovmr_amd import cli, trainer
    result, argv = sys.argv[1], sys.argv[2:]
    fitted = {}
    keep = trainer.LinearProbe._fitted

    def spy(self, state, search=None):                          # every rank fits; only rank 0 writes the file
        fitted.update(W=state.W.clone(), b=state.b.clone(), n_iter=state.n_iter)
        return keep(self, state, search)
    trainer.LinearProbe._fitted = spy
    buf = io.StringIO()
    try:
        with redirect_stdout(buf):
            results = cli.main(argv)
    finally:
        sys.stdout.write(buf.getvalue())                     # (the launcher keeps it next to stderr for a failing rank)
    torch.save(dict(fitted, results=results, stdout=buf.getvalue()), result)


if __name__ == "__main__":
    main()
