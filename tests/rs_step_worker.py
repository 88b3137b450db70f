"""Worker of tests/test_gpu_rs_step.py: two ranks (gloo) on ONE GPU run a step object's run() for a range-separated hybrid
to convergence on the mixed-kernel table set, and every rank writes its energies, iteration count and trace."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(out_prefix, names):
    import helfem_amd as hf
    from helfem_amd import parallel
    import rs_step_common as common
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank, local_rank, world = parallel.init(backend="gloo" if world > 1 else None)
    allred = parallel.allreduce_sum_ if world > 1 else None
    xblocks = parallel.broadcast_block_slots_ if world > 1 else None
    out = {}
    for name in names:
        step, S, Enucr = common.make_step(hf, name, rank=rank, nranks=world)
        out[name] = step.run(S, Enucr=Enucr, allreduce=allred, exchange_blocks=xblocks)
        out[name]["mix"] = bool(step.mix)
    json.dump(out, open("%s.rank%d.json" % (out_prefix, rank), "w"))
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2].split(","))
