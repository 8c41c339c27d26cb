"""profiles/head_variant_errors.md from the log of tests/test_gpu_head_variants.py.

    GM_HEAD_VARIANT_LOG=errors.tsv python -m pytest -m gpu tests/test_gpu_head_variants.py
    python tools/head_variant_profile.py errors.tsv > profiles/head_variant_errors.md

One line per (kernel, key, band): the largest scaled error of the HIP result and of the fp32 torch-CPU result against the
staged fp64 reference over every case, mode, activation and output of that group, and the groups that passed only by the
4-ulp floor."""
import collections
import sys

ULP = 2.0 ** -23


def main(path):
    groups = collections.OrderedDict()
    n = 0
    for line in open(path):
        kernel, key, mode, act, shape, what, band, e_hip, e_cpu, scale, verdict = line.rstrip("\n").split("\t")
        g = groups.setdefault((kernel, key, band), dict(n=0, hip=(0.0, ""), cpu=0.0, ratio=0.0, floor=[], fail=[]))
        e_hip, e_cpu = float(e_hip), float(e_cpu)
        where = "%s %s %s %s" % (what, mode, act, shape)
        g["n"] += 1
        n += 1
        if e_hip >= g["hip"][0]:
            g["hip"] = (e_hip, where)
        g["cpu"] = max(g["cpu"], e_cpu)
        g["ratio"] = max(g["ratio"], e_hip / (2.0 * e_cpu + ULP))
        if verdict != "close64":
            g["floor" if verdict == "floor" else "fail"].append("%s (e_hip %.3e, e_cpu %.3e)" % (where, e_hip, e_cpu))
    print("# Loss variants on the critic-head kernels: measured errors\n")
    print("From the log of `tests/test_gpu_head_variants.py` on an MI355X (%d comparisons; regenerate with" % n)
    print("`tools/head_variant_profile.py`).  Errors are scaled: per-row arrays by the largest reference magnitude of")
    print("their band, the loss by `inv_b * sum |row term|`, gb2 by `sum |dS|`, other arrays by their largest reference")
    print("magnitude.  `e_hip`: HIP against the staged fp64 reference; `e_cpu`: fp32 torch CPU against it; both the")
    print("largest over the group's cases (shapes, modes, activations, outputs).  `of bound`: the largest")
    print("`e_hip / (2 e_cpu + 1 ulp)` of any single comparison (1 ulp = 2^-23 = 1.19e-07); above 1 a comparison needs the")
    print("floor of 4 ulp.  Band `all`: scalars and reduced arrays (loss, gw2, gb2, gW1, gb1, Adam state, Fisher's state).\n")
    print("Kernels: `gan_loss` ops.gan_loss; `head_pair` head_fwd_loss + head_bwd (`+pen` penalty rows, `+ld` strided views);")
    print("`fold_critic` / `unfolded_critic` the critic step with the head folded into the weight-gradient launch / as")
    print("head_fwd_loss + that launch; `fold_two_phase` the RaGAN / Fisher folded critic step; `fold_generator` the folded")
    print("generator step.\n")
    floors = [(k, f) for k, g in groups.items() for f in g["floor"]]
    fails = [(k, f) for k, g in groups.items() for f in g["fail"]]
    print("Comparisons that needed the 4-ulp floor: %s" % (len(floors) or "none"))
    for k, f in floors:
        print("- %s / %s / %s: %s" % (k + (f,)))
    print("\nComparisons beyond the floor (findings): %s\n" % (len(fails) or "none"))
    for k, f in fails:
        print("- %s / %s / %s: %s" % (k + (f,)))
    print("| kernel | key | band | comparisons | e_hip | e_cpu | of bound | worst at |")
    print("|---|---|---|---|---|---|---|---|")
    for (kernel, key, band), g in groups.items():
        print("| %s | %s | %s | %d | %.2e | %.2e | %.2f | %s |" % (kernel, key, band, g["n"], g["hip"][0], g["cpu"], g["ratio"],
                                                                g["hip"][1]))


if __name__ == "__main__":
    main(sys.argv[1])
