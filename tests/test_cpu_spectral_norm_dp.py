"""Two gloo ranks of Pix2Pix with a spectrally normalised PatchGAN (-m "not gpu", the torch-CPU stand-in of the C ABI): `weight_u` and
`weight_v` are rank-local buffers that no collective touches, yet after the steps both ranks hold the same bits -- each rank sees the
same parameters (exchanged gradients, same Adam) and runs the same fixed-order arithmetic on them.  The ranks start from DIFFERENT
vectors and weights; the rank-0 start-state broadcast (sync_replicas) must cover the buffers too."""
import os

import torch
import torch.multiprocessing as mp

import emul_backend
import test_cpu_spectral_norm as C
import test_gpu_spectral_norm as G
from oracle import detrand, ref_harness

KW = dict(model="pix2pix", batch=4, crop=64, n_blocks=1, ngf=16, ndf=16, pixel_weight=100.0)
STEPS = 2


def _worker(rank, world, port, tmp, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    try:
        torch.set_num_threads(4)
        emul_backend.install()
        from trainner_amd import dp as dpmod, ops
        from trainner_amd.models import create_model
        from trainner_amd.options import options
        ops.sn_forward, ops.sn_backward = C.emul_sn_forward, C.emul_sn_backward
        dpmod.BUCKET_FLOATS = 20_000              # several buckets per network
        yml = G.add_key_to_network_D(ref_harness.i2i_yaml(name="dp_sn", out_root=os.path.join(tmp, "r%d" % rank), gpu_ids="[0]", **KW))
        model = create_model(options.parse(yml, is_train=True), verbose=False)
        assert model.dp.active and model.dp.world_size == world and model.netD._has_sn
        for net, seed in ((model.netG, 101), (model.netD, 202)):
            net.load_state_dict(detrand.fill_state_dict_({k: v.clone() for k, v in net.state_dict().items()}, seed + 400 * rank))
        model.sync_replicas()
        for s in range(1, STEPS + 1):
            A = detrand.uniform((KW["batch"], 3, 64, 64), 170 + s, -1.0, 1.0)      # every rank is fed the GLOBAL batch and takes its shard
            B = detrand.uniform((KW["batch"], 3, 64, 64), 180 + s, -1.0, 1.0)
            model.feed_data({"A": A, "B": B, "A_path": ["a"] * KW["batch"]})
            model.optimize_parameters(s)
        path = os.path.join(tmp, "rank%d.pt" % rank)
        torch.save({k: v.detach().clone() for k, v in model.netD.state_dict().items()}, path)
        q.put((rank, path))
    except Exception as e:                           # pragma: no cover
        import traceback
        q.put((rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
    finally:
        import torch.distributed as dist
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_ranks_keep_u_and_v_bit_identical(tmp_path):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35000 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in range(2):
        assert res[r].endswith(".pt"), res[r]
        res[r] = torch.load(res[r], weights_only=False)
    keys = list(res[0])
    assert any(k.endswith("weight_u") for k in keys) and any(k.endswith("weight_orig") for k in keys)
    start = detrand.fill_state_dict_({k: v.clone() for k, v in res[0].items()}, 202)
    for k in keys:
        assert torch.equal(res[0][k], res[1][k]), k
        assert not torch.equal(res[0][k], start[k]), k                  # (the steps moved every tensor, the vectors included)
