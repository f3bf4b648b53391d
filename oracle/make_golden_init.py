"""tests/golden/init_weights.json: the reference's initial weights after `set_random_seed(7)`, one SHA-256 per tensor.

TEST INFRASTRUCTURE ONLY (build container: reads /root/reference).  Usage:  python -m oracle.make_golden_init

For every case of CASES the reference's own options.parse / create_model builds the model (oracle/ref_harness.build_reference_model)
and every state_dict entry of the networks named is stored as [key, shape, dtype, sha256 of its bytes], in state_dict order.
tests/test_cpu_init_reference.py builds the engine from the same options and seed and compares it with this fixture bit for bit;
where the reference checkout is present it also compares with the live reference.
"""
import hashlib
import json
import os

from . import ref_harness as R

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
OUT = os.path.join(GOLDEN, "init_weights.json")
SEED = 7

CASES = {
    "esrgan": (R.esrgan_yaml, dict(nb=2, batch=2, crop=64, d_nf=16), ("G", "D")),
    "esrgan_unet_d": (R.esrgan_yaml, dict(nb=1, batch=2, crop=64, d_nf=16, d_type="unet"), ("G", "D")),
    "srresnet_psnr": (R.esrgan_yaml, dict(nb=2, batch=2, crop=64, model_G="sr_resnet", gan=False, feature=False), ("G",)),
    "cyclegan": (R.i2i_yaml, dict(model="cyclegan", batch=1, crop=64, n_blocks=2, ngf=16, ndf=16), ("G_A", "G_B", "D_A", "D_B")),
    "pix2pix_unet": (R.i2i_yaml, dict(model="pix2pix", batch=2, crop=128, ngf=16, ndf=16, norm_G="batch", which_G="unet_128"), ("G", "D")),
}


def digest(t):
    """[shape, dtype, sha256 of the tensor's bytes] of a state_dict entry."""
    a = t.detach().cpu().contiguous().numpy()
    return [list(a.shape), str(a.dtype), hashlib.sha256(a.tobytes()).hexdigest()]


def reference_digests(case, out_root):
    make, kw, nets = CASES[case]
    _, ref = R.build_reference_model(make(name="init", out_root=out_root, **kw), seed=SEED)
    return ref, {n: [[k] + digest(v) for k, v in getattr(ref, "net" + n).state_dict().items()] for n in nets}


def main():
    import tempfile
    out = {case: reference_digests(case, tempfile.mkdtemp(prefix="tnr_init_"))[1] for case in CASES}
    with open(OUT, "w") as f:
        json.dump(out, f, indent=0)
    for case, nets in out.items():
        print(case, {n: len(v) for n, v in nets.items()})
    print(OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
