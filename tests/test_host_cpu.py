"""CPU-side checks (no GPU): the C-ABI library loads and exports every declared symbol, host
helpers are bit-exact against torch, drop-in modules expose the reference's surface, fast-path
selection logic, and the product fails loudly instead of computing on CPU."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(os.path.dirname(HERE), "generative_models_amd", "src")
sys.path.insert(0, SRC)
sys.path.insert(0, HERE)

import abi_header  # noqa: E402
from generative_models_amd import _lib, engine, ops, trainers  # noqa: E402


def test_library_loads_and_exports_every_declared_symbol():
    lib = _lib.load()
    declared = abi_header.declared_symbols()
    assert len(declared) >= 52
    for name in declared:
        assert hasattr(lib, name), name
        assert name in _lib._SIGNATURES, "declared in gm_hip.h but not bound: " + name
    for name in _lib._SIGNATURES:
        assert name in declared, "bound but not declared in gm_hip.h: " + name
    assert lib.gm_arch() == b"gfx950" and lib.gm_version() >= 100


def test_bad_arguments_are_rejected_without_a_gpu():
    lib = _lib.load()
    rc = lib.gm_linear_fwd(None, None, 0, _lib.NO_SLOT, None, None, None, 0, 0, 0, 0, 0)
    assert rc == _lib.GM_EINVAL and b"bad argument" in lib.gm_last_error()
    with pytest.raises(_lib.GMError):
        _lib.call("gm_adam", None, None, None, None, None, 0, None, _lib.NO_SLOT, 0.9, 0.999, 1e-8,
                  0.0, 0.0)


@pytest.mark.parametrize("seed", [0, 1, 12345, 2 ** 40 + 17, 2 ** 63 - 5])
@pytest.mark.parametrize("n,B", [(50000, 256), (50000, 1024), (160, 16), (1000, 1000), (10, 10), (7, 1)])
def test_randperm_prefix_bit_exact(seed, n, B):
    g = torch.Generator()
    g.manual_seed(seed)
    ref = torch.randperm(n, generator=g)[:B].numpy()
    assert np.array_equal(ops.randperm_prefix(seed, n, B), ref)


def test_sampler_protocol_matches_dataloader_bit_exact():
    """engine.draw_sampler_indices == the batch the reference's DataLoader would yield, and it
    leaves the global generator in the same state."""
    data = torch.arange(500, dtype=torch.float32).reshape(500, 1)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, torch.zeros(500)),
                                         batch_size=32, shuffle=True)
    torch.manual_seed(11)
    ref = [next(iter(loader))[0].reshape(-1).long().numpy() for _ in range(4)]
    ref_state = torch.get_rng_state()
    torch.manual_seed(11)
    idx = np.empty(32, dtype=np.int64)
    for r in ref:
        engine.draw_sampler_indices(500, 32, idx)
        assert np.array_equal(idx, r)
    assert torch.equal(ref_state, torch.get_rng_state())


@pytest.mark.parametrize("seed", [0, 11])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("D_steps", [1, 2])
def test_nsgan_order_draws_match_the_reference_loop_bit_exact(D_steps, k, seed):
    """ring_engine.nsgan_order_draws == what ns_gan.py's loop takes from the global generator in k iterations: per
    critic step next(iter(loader)) and randn(B, Z), then the generator step's randn(B, Z); ring rows i * D_steps + j
    and i, rows past the k iterations untouched, and the generator left in the same state."""
    from generative_models_amd import ring_engine
    n, B, Z = 40, 8, 4
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.arange(n), torch.arange(n)),
                                         batch_size=B, shuffle=True)
    torch.manual_seed(seed)
    ref_idx, ref_zD, ref_zG = [], [], []
    for _ in range(k):
        for _ in range(D_steps):
            ref_idx.append(next(iter(loader))[0])
            ref_zD.append(torch.randn(B, Z))
        ref_zG.append(torch.randn(B, Z))
    ref_state = torch.get_rng_state()
    torch.manual_seed(seed)
    idx = torch.full((k * D_steps + 1, B), -1, dtype=torch.int64)
    zD, zG = torch.full((k * D_steps + 1, B, Z), -9.0), torch.full((k + 1, B, Z), -9.0)
    ring_engine.nsgan_order_draws(n, B, D_steps, k, idx, zD, zG)
    assert torch.equal(idx[:-1], torch.stack(ref_idx)) and bool((idx[-1] == -1).all())
    assert torch.equal(zD[:-1], torch.stack(ref_zD)) and bool((zD[-1] == -9).all())
    assert torch.equal(zG[:-1], torch.stack(ref_zG)) and bool((zG[-1] == -9).all())
    assert torch.equal(ref_state, torch.get_rng_state())


def test_epoch_order_matches_dataloader():
    data = torch.arange(100, dtype=torch.float32).reshape(100, 1)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(data, torch.zeros(100)),
                                         batch_size=16, shuffle=True)
    torch.manual_seed(5)
    ref = torch.cat([b[0].reshape(-1) for b in loader]).long()
    st = torch.get_rng_state()
    torch.manual_seed(5)
    assert torch.equal(trainers._epoch_order(loader), ref)
    assert torch.equal(st, torch.get_rng_state())


def test_adam_schedule_matches_torch_scalars():
    s = ops.adam_schedule(2e-4, 5)
    for i, step in enumerate(range(1, 6)):
        bc1, bc2 = 1 - 0.9 ** step, 1 - 0.999 ** step
        assert s[i, 0] == np.float32(2e-4 / bc1) and s[i, 1] == np.float32(bc2 ** 0.5)


def test_dropin_surface_and_state_dict_keys():
    import ns_gan, w_gp_gan, be_gan, info_gan, vae, f_gan, utils  # noqa: F401
    m = ns_gan.NSGAN(784, 400, 20)
    assert list(m.state_dict()) == ["G.linear.weight", "G.linear.bias", "G.generate.weight",
                                    "G.generate.bias", "D.linear.weight", "D.linear.bias",
                                    "D.discriminate.weight", "D.discriminate.bias"]
    assert (m.z_dim, m.shape, m.image_size, m.hidden_dim, m.output_dim) == (20, 28, 784, 400, 1)
    assert sum(p.numel() for p in m.parameters()) == 637185
    assert list(be_gan.BEGAN(784, 400, 20).state_dict())[4:] == [
        "D.encoder.weight", "D.encoder.bias", "D.decoder.weight", "D.decoder.bias"]
    assert "D.discriminator.weight" in info_gan.InfoGAN(784, 400, 20, 10, 10).state_dict()
    assert sum(p.numel() for p in vae.VAE().parameters()) == 652824
    import ae
    assert sum(p.numel() for p in ae.Autoencoder().parameters()) == 50992       # SURVEY A.1 PROBE
    assert list(ae.Autoencoder().state_dict().keys()) == [
        "encoder.linear.weight", "encoder.linear.bias", "decoder.linear.weight", "decoder.linear.bias"]
    for name in ("Encoder", "Decoder", "Autoencoder", "AutoencoderTrainer", "get_data", "to_cuda"):
        assert hasattr(ae, name), name
    for name in ("Generator", "Discriminator", "NSGAN", "NSGANTrainer", "to_cuda", "to_var", "get_data"):
        assert hasattr(ns_gan, name)
    assert hasattr(f_gan, "Divergence") and hasattr(info_gan, "Q")
    with pytest.raises(AssertionError):
        f_gan.Divergence("not-a-divergence")


@pytest.mark.parametrize("pipelined", [True, False])
def test_epoch_loop_enqueues_the_next_epoch_before_it_reads_the_previous_one_back(pipelined, monkeypatch, capsys):
    """trainers._train on a stand-in engine (no GPU): with one rank and no viz, epoch e+1's run() comes BEFORE epoch e's
    losses(after=mark of epoch e); histories and progress lines come out in epoch order either way; an error in a later
    run() still records the finished epoch; GM_PIPELINE_EPOCHS=0 reads back before the next epoch is enqueued."""
    import ns_gan
    from oracle import port
    loaders = port.synthetic_loaders(16, n_train=160, n_val=48, n_test=48, image_shape=(1, 8, 8))
    tr = ns_gan.NSGANTrainer(ns_gan.NSGAN(64, 48, 8), *loaders)
    calls = []

    class Engine:
        world = 1
        fail_at = None

        def configure(self, n, *a, **k):
            calls.append(("configure", n))

        def run(self, n, it_start=0, horizon=None):
            if self.fail_at == it_start:
                raise RuntimeError("boom")
            calls.append(("run", it_start, n, horizon))

        def mark(self):
            calls.append(("mark",))
            return "mark%d" % sum(1 for c in calls if c[0] == "mark")

        def losses(self, it0, it1, after=None):
            calls.append(("losses", it0, it1, after))
            return [float(it0)] * (it1 - it0), [float(it0) + 0.5] * (it1 - it0)

    eng = Engine()
    monkeypatch.setattr(tr, "_get_engine", lambda: eng)
    if not pipelined:
        monkeypatch.setenv("GM_PIPELINE_EPOCHS", "0")
    tr.train(3)
    names = [(c[0],) + ((c[1],) if c[0] in ("run", "losses") else ()) for c in calls]
    if pipelined:
        assert names == [("configure",), ("run", 0), ("mark",), ("run", 10), ("mark",), ("losses", 0), ("run", 20), ("mark",),
                         ("losses", 10), ("losses", 20)]
        assert [c[3] for c in calls if c[0] == "losses"] == ["mark1", "mark2", "mark3"]
    else:
        assert names == [("configure",), ("run", 0), ("losses", 0), ("run", 10), ("losses", 10), ("run", 20), ("losses", 20)]
        assert all(c[3] is None for c in calls if c[0] == "losses")
    assert all(c[3] == 30 for c in calls if c[0] == "run")               # horizon: the whole train() call
    assert tr.Glosses == [0.0] * 10 + [10.0] * 10 + [20.0] * 10 and tr.Dlosses[10] == 10.5 and tr.num_epochs == 3
    out = capsys.readouterr().out
    assert [ln[:10] for ln in out.strip().splitlines()] == ["Epoch[1/3]", "Epoch[2/3]", "Epoch[3/3]"]
    # an error in epoch 3's run(): epochs 1 and 2 are on record when it surfaces
    tr2 = ns_gan.NSGANTrainer(ns_gan.NSGAN(64, 48, 8), *loaders)
    eng2 = Engine()
    eng2.fail_at = 20
    monkeypatch.setattr(tr2, "_get_engine", lambda: eng2)
    with pytest.raises(RuntimeError):
        tr2.train(3)
    assert tr2.num_epochs == 2 and len(tr2.Glosses) == 20


def test_same_seed_gives_reference_initial_weights():
    """nn.Linear construction order == the reference's (G.linear, G.generate, D.linear, D...)."""
    import ns_gan
    from oracle import port
    torch.manual_seed(1234)
    a = ns_gan.NSGAN(64, 48, 8).state_dict()
    b = port.build("ns", 64, 48, 8).state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_fast_path_selection_and_no_cpu_compute():
    import ns_gan
    from oracle import port
    loaders = port.synthetic_loaders(16, n_train=160, n_val=48, n_test=48, image_shape=(1, 8, 8))
    tr = ns_gan.NSGANTrainer(ns_gan.NSGAN(64, 48, 8), *loaders)
    assert tr._stock()

    class Mine(ns_gan.NSGANTrainer):
        def train_G(self, images):
            return super().train_G(images)
    assert not Mine(ns_gan.NSGAN(64, 48, 8), *loaders)._stock()
    seq = torch.utils.data.DataLoader(loaders[0].dataset, batch_size=16, shuffle=False)
    assert not ns_gan.NSGANTrainer(ns_gan.NSGAN(64, 48, 8), seq, None, None)._stock()
    if not torch.cuda.is_available():
        with pytest.raises(_lib.GMError):
            tr.train(1)                                   # no GPU -> loud failure, never CPU math
        with pytest.raises(_lib.GMError):
            tr.model.G(torch.zeros(2, 8))


def test_flat_params_pack_and_alias():
    lin_a, lin_b = torch.nn.Linear(5, 3), torch.nn.Linear(3, 7)
    w0 = lin_a.weight.detach().clone()
    fp = engine.FlatParams([lin_a.weight, lin_a.bias, (lin_b.weight, lin_b.bias)], "cpu")
    assert fp.offsets == [0, 16, 20, 41] and fp.n == 48
    assert torch.equal(lin_a.weight.data, w0)
    fp.flat[0] = 42.0
    assert lin_a.weight.data[0, 0].item() == 42.0 and fp.still_bound()


def test_bench_kernel_names_match_the_committed_rocprof_summary():
    """bench.py names the kernel instantiation of every GEMM launch shape of the step (it mirrors
    the library's tile / schedule selection); those names must be the ones rocprofv3 recorded in
    the committed round summary, and the bench line's dominant kernel must be one of them."""
    import csv
    import importlib.util
    import json
    root = os.path.dirname(HERE)
    spec = importlib.util.spec_from_file_location("gm_bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rnd = bench.PROFILE_ROUND                  # the round whose kernels bench.py mirrors
    stats = os.path.join(root, "profiles", rnd + "_nsgan_b256_kernel_stats.csv")
    if not os.path.isfile(stats):
        pytest.skip("the %s rocprofv3 summary is not committed yet" % rnd)
    rows = list(csv.DictReader(open(stats)))
    profiled = {r["kernel"] for r in rows}
    names = {bench.gemm_variant(*shape) for shape in bench.gemm_shapes(256, fold_head=bench.FOLD_HEAD_DEFAULT)}
    assert len(names) >= 6
    for n in names:
        assert n in profiled, "bench names %r, rocprofv3 saw %s" % (n, sorted(profiled)[:12])
    line = json.loads(open(os.path.join(root, "profiles", rnd + "_bench_default.json")).read().strip().splitlines()[-1])
    assert line["roofline"]["kernel"] in names
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in line["roofline"]
    # no silent `traffic: null`: the dominant kernel of the headline and of every configuration that has a
    # roofline entry must be listed in the committed PMC pass it names
    assert line["roofline"]["traffic"] and line["roofline"]["traffic_source"].startswith("profiles/" + rnd)
    for c in line["config"].get("other_configs", line.get("configs", [])):      # (round <= 4 records: top level)
        r = c.get("roofline")
        if r is not None and "kernel" in r:                  # (the variants outside BASELINE.json carry a STEP-level roofline)
            assert r["traffic"] and os.path.isfile(os.path.join(root, r["traffic_source"])), c["workload"]
        elif r is not None:
            assert r["step_frac"] > 0 and r["flop_per_image"] > 0 and os.path.isfile(os.path.join(root, r["profile"])), c["workload"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in line["cpu_baseline"]
    avg = {r["kernel"]: float(r["avg_us"]) for r in rows}
    # the live HIP-event duration and the profiler's average of the same kernel agree (different boxes:
    # this round's boxes differ by up to 8 % on the same kernel, and the profiler adds 0.3-0.8 us)
    assert abs(avg[line["roofline"]["kernel"]] - line["roofline"]["avg_launch_us"]) <= 1.5
    # and its MFMA-busy fraction resolves against the committed SQ counter pass (which may predate the last
    # template flag of the kernel's printed name)
    busy = bench.mfma_busy_frac(line["roofline"]["kernel"], line["roofline"]["avg_launch_us"], 2300)
    assert busy is not None and 0.05 < busy < 1.0, busy


@pytest.mark.parametrize("tag", ["wgp_b256", "ns_b1024", "vae_b512"])
def test_bench_kernel_names_of_the_other_configurations_match_their_summaries(tag):
    """The per-configuration roofline entries are built from bench.py's mirror of the library's kernel choice
    for that configuration's launch shapes (WGAN-GP incl. the 3B-row forward on 48x32 tiles and the stacked
    weight gradient, bs=1024 incl. the interleaved-fragment instantiations, the VAE's epilogue forms): every name
    must be one rocprofv3 recorded in the committed summary of that configuration."""
    import csv
    import importlib.util
    root = os.path.dirname(HERE)
    spec = importlib.util.spec_from_file_location("gm_bench", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    stats = os.path.join(root, "profiles", "%s_%s_kernel_stats.csv" % (bench.PROFILE_ROUND, tag))
    if not os.path.isfile(stats):
        pytest.skip("no committed summary for " + tag)
    profiled = {r["kernel"] for r in csv.DictReader(open(stats))}
    shapes = {"wgp_b256": lambda: bench.gemm_shapes_wgp(256), "ns_b1024": lambda: bench.gemm_shapes(1024, fold_head=False),
              "vae_b512": lambda: bench.gemm_shapes_vae(512)}[tag]()
    names = {bench.gemm_variant(*sh[:5]) for sh in shapes}
    assert len(names) >= 5
    for n in names:
        assert n in profiled, "bench names %r for %s, rocprofv3 saw %s" % (n, tag, sorted(profiled)[:14])


@pytest.mark.parametrize("kind", ["normal", "uniform"])
@pytest.mark.parametrize("B,W,r0,r1", [(2048, 20, 256, 512), (2048, 20, 0, 256), (512, 20, 384, 512),
                                       (256, 784, 64, 128), (2048, 1, 256, 512), (48, 8, 16, 32),
                                       (24, 10, 8, 16), (7, 3, 2, 4)])
def test_draw_rows_is_a_bit_exact_slice_of_the_full_draw(kind, B, W, r0, r1):
    """Data-parallel ranks materialise only their own rows of each noise tensor: the rows must be
    bit-identical to the same rows of the full draw and the global generator must end where the
    full draw would have left it (unaligned shapes fall back to the full draw)."""
    torch.manual_seed(11); torch.empty(5).random_()
    full = getattr(torch.empty(B, W), kind + "_")()
    ref_state = torch.get_rng_state().clone()
    torch.manual_seed(11); torch.empty(5).random_()
    part = torch.full((B, W), -7.0)
    engine.draw_rows(part, r0, r1, kind)
    assert torch.equal(part[r0:r1], full[r0:r1])
    assert torch.equal(ref_state, torch.get_rng_state())
    nxt = torch.randn(33)
    torch.set_rng_state(ref_state)
    assert torch.equal(nxt, torch.randn(33))


def test_mt19937_skip_equals_discarding_outputs():
    for n in (1, 623, 624, 625, 5120, 123457):
        torch.manual_seed(7); torch.empty(3).random_()
        torch.empty(n, dtype=torch.int32).random_()            # one 32-bit output per element
        ref = torch.get_rng_state().clone()
        torch.manual_seed(7); torch.empty(3).random_()
        engine._rng_skip(n)
        assert torch.equal(ref, torch.get_rng_state()), n


@pytest.mark.parametrize("variant", ["ns", "wgp"])
def test_dp_ranks_replay_the_global_draw_protocol(variant):
    """_draw_D / _draw_G on rank r of a 4-rank job: own rows bit-identical to the single-process
    draws, identical sampling indices, identical generator position afterwards."""
    from types import SimpleNamespace
    B, Z, N, R = 64, 20, 5000, 3

    def stage():
        s = dict(idx=torch.zeros(R, B, dtype=torch.int64), zD=torch.full((R, B, Z), -9.0),
                 zG=torch.full((R, B, Z), -9.0), eps=torch.full((R, B), -9.0))
        s["idx_np"] = s["idx"].numpy()
        return s

    def replay(world, rank):
        eng = SimpleNamespace(N=N, B=B, Bl=B // world, world=world, rank=rank, variant=variant)
        eng._noise = lambda dst, kind: engine.GANEngine._noise(eng, dst, kind)
        torch.manual_seed(99)
        s = stage()
        for k in range(R):
            engine.GANEngine._draw_D(eng, s, k)
            engine.GANEngine._draw_G(eng, s, k)
        return s, torch.get_rng_state()

    full, full_state = replay(1, 0)
    for rank in range(4):
        s, state = replay(4, rank)
        r0, r1 = rank * 16, rank * 16 + 16
        assert torch.equal(s["idx"], full["idx"])
        for key in ("zD", "zG") + (("eps",) if variant == "wgp" else ()):
            assert torch.equal(s[key][:, r0:r1], full[key][:, r0:r1]), (key, rank)
            assert bool((s[key][:, :r0] == -9).all()) and bool((s[key][:, r1:] == -9).all())
        assert torch.equal(state, full_state)


@pytest.mark.parametrize("R,graph_iters", [(128, 32), (25, 32), (7, 8), (128, 8), (16, 32)])
def test_launch_planner_invariants(R, graph_iters):
    """GANEngine._plan: pieces are powers of two <= min(graph_iters, R), cover the run exactly, never
    cross the end of the ring (a stage-in copies contiguous slots); a cold run starts with a piece of
    at most FIRST_PIECE iterations and no piece exceeds 4x what precedes it."""
    class E:
        pass
    e = E()
    e.graph_iters, e.R, e.FIRST_PIECE = graph_iters, R, 2
    plan = lambda it, n, cold: engine.GANEngine._plan(e, it, n, cold)
    cap = min(graph_iters, R)
    for it in (0, 5, R - 1, R, 3 * R + 2):
        for n in (0, 1, 2, 3, 20, 25, 64, 200, 2000):
            for cold in (False, True):
                p = plan(it, n, cold)
                assert sum(p) == n and all(x >= 1 and x & (x - 1) == 0 and x <= cap for x in p), (it, n, cold, p)
                pos, done = it, 0
                for x in p:
                    assert pos % R + x <= R, (it, n, cold, p)      # no ring wrap inside a piece
                    if cold:
                        assert x <= (e.FIRST_PIECE if done == 0 else max(1, 4 * done)), (it, n, p)
                    pos += x
                    done += x
    if R >= 32 and graph_iters >= 16:
        assert plan(5, 20, True) == [2, 2, 16]        # the driver's 20-step run


def test_no_function_of_the_package_reads_a_name_its_module_does_not_define():
    """tools/undefined_names.py over every module of the package: a method moved between modules (engine.py ->
    gan_steps.py / vae_engine.py / began_engine.py) must not leave a global behind that only a rarely run path reads."""
    import subprocess
    import sys
    root = os.path.dirname(HERE)
    mods = ["generative_models_amd." + m for m in ("engine", "gan_steps", "vae_engine", "began_engine", "trainers", "ops",
                                                   "ops_fused", "dp", "viz", "_lib", "_build", "ring_engine")]
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "undefined_names.py")] + mods,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.parametrize("variant,B,Z,d,expect", [("ns", 256, 20, 1, (512, 128)), ("wgp", 256, 20, 1, (512, 128)),
                                                   ("ns", 512, 20, 1, (256, 64)), ("ns", 1024, 20, 1, (128, 32)),
                                                   ("wgp", 256, 20, 5, (128, 32)), ("dra", 256, 20, 1, (64, 32)),
                                                   ("info", 256, 40, 1, (256, 64))])
def test_ring_and_graph_size_follow_the_bytes_of_draws_per_iteration(variant, B, Z, d, expect, monkeypatch):
    """GANEngine._ring_and_graph_size: 128 iterations per graph on a 512-slot ring up to 64 KB of host draws per
    iteration, 64 / 256 up to 128 KB, else 32 / 128; DRAGAN keeps <= 64 slots; GM_RING / GM_GRAPH_ITERS fix either."""
    class E:
        pass
    e = E()
    e.variant, e.B, e.Z, e.I = variant, B, Z, 784
    monkeypatch.delenv("GM_RING", raising=False)
    monkeypatch.delenv("GM_GRAPH_ITERS", raising=False)
    assert engine.GANEngine._ring_and_graph_size(e, d) == expect
    monkeypatch.setenv("GM_RING", "96")
    assert engine.GANEngine._ring_and_graph_size(e, d) == (min(96, 64) if variant == "dra" else 96, 32)
    monkeypatch.setenv("GM_GRAPH_ITERS", "8")
    assert engine.GANEngine._ring_and_graph_size(e, d)[1] == 8


@pytest.mark.parametrize("record", ["r02_bench_default.json", "r02_bench_steps20_warmup5.json"])
def test_committed_bench_records_follow_the_contract(record):
    """The bench lines committed under profiles/ carry every key of the driver's contract with the
    right types, the roofline / cpu_baseline objects, and the configs 3/4/5 section."""
    import json
    root = os.path.dirname(HERE)
    line = json.loads(open(os.path.join(root, "profiles", record)).read().strip().splitlines()[-1])
    for key, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int),
                     ("warmup", int), ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str),
                     ("dtype", str), ("data", str), ("config", dict), ("roofline", dict), ("cpu_baseline", dict)):
        assert isinstance(line[key], typ), (key, type(line[key]))
    assert "vs_baseline" in line and line["vs_baseline"] is None        # BASELINE.md holds no number for this metric
    assert line["n_gpus"] == 1 and line["dtype"] == "f32" and line["scaling"] == "weak" and line["data"] == "synthetic"
    assert "workload" in line["config"] and "model" not in line["config"]
    assert abs(line["value"] - 256 / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    r = line["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and (r["traffic"] is None or r["traffic"] > 0)
    c = line["cpu_baseline"]
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    if record == "r02_bench_steps20_warmup5.json":
        assert line["steps"] == 20 and line["warmup"] == 5          # the driver's command
    names = " | ".join(e["workload"] for e in line.get("configs", []))
    for needle in ("WGAN-GP", "NSGAN MNIST bs=1024", "LSGAN MNIST bs=1024", "VAE MNIST bs=512"):
        assert needle in names, (needle, names)


def _kernel_resources():
    import importlib.util
    root = os.path.dirname(HERE)
    spec = importlib.util.spec_from_file_location("gm_kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not (os.path.isfile(kr.LIB) and kr.tools_available()):
        pytest.skip("needs the built libgm_hip.so and the ROCm LLVM binutils")
    return kr


def test_kernel_register_and_code_size_baseline():
    """Every kernel of the built library against profiles/kernel_resources.json (VGPR / SGPR / spills / LDS / scratch /
    code bytes, read from the code objects inside the .so).  Round 3's dominant forward kernel got 6 % slower across a
    round in which nothing in it was meant to change -- template flags and sibling instantiations accumulating around
    it.  A change here is not a failure of the code, it is a change that has to be LOOKED at: refresh the baseline with
    `python tools/kernel_resources.py --write` in the same commit (and say why in its message)."""
    kr = _kernel_resources()
    table = kr.kernel_table()
    base = json.load(open(kr.BASELINE))
    d = kr.diff(table, base)
    assert not d, "kernel resources moved against profiles/kernel_resources.json:\n" + "\n".join(d[:40])
    # the hot kernels stay inside their occupancy class and out of scratch
    for k, r in table.items():
        assert r["scratch"] == 0 or "bir_mmd_kernel" in k, (k, r)
        if k.startswith("gemm16_"):
            assert r["vgpr"] <= 128, (k, r)          # 1024-thread workgroups: 4 waves per SIMD
        if k.startswith("gemm_lds_kernel"):
            assert r["vgpr"] <= 256, (k, r)          # 512-thread workgroups: 2 waves per SIMD


def test_committed_counter_passes_name_kernels_the_library_contains():
    """Every kernel named in a committed PMC / SQ counter pass of the round bench.py reads (profiles/<round>_*_pmc_traffic
    .json, *_sq_pmc.json) must exist in the built library: a pass taken before a kernel was renamed or re-templated
    would silently give the bench line `traffic: null` (or, worse, a number of another kernel)."""
    import glob
    import importlib.util
    kr = _kernel_resources()
    root = os.path.dirname(HERE)
    spec = importlib.util.spec_from_file_location("gm_bench2", os.path.join(root, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    files = glob.glob(os.path.join(root, "profiles", bench.PROFILE_ROUND + "_*_pmc_traffic.json")) + \
        glob.glob(os.path.join(root, "profiles", bench.PROFILE_ROUND + "_*_sq_pmc.json"))
    if not files:
        pytest.skip("no committed counter pass of round %s yet" % bench.PROFILE_ROUND)
    have = set(kr.kernel_table())
    for f in files:
        for key in json.load(open(f)):
            name = key.split("|")[0]
            if name.startswith(("gemm", "head_", "gan_loss", "adam_", "stage_in", "ar_", "vae_", "std_", "gp_", "interp",
                                "sum_finalize", "gather_rows", "tick", "dragan", "began", "info_q", "bir_", "l1_rows", "sqerr")):
                assert name in have, "%s names %r, which the built library does not contain" % (os.path.basename(f), name)


def test_environment_switchboard_is_pinned():
    """the product is steered by at most 15 GM_* environment switches, each with an agreement test
    under tests/ (bitwise or to-rounding, named here); everything else that rounds 1 - 5 kept for A/B runs is gone (the
    slower arms' measurements are in profiles/r0*_experiments.md).  A new os.environ / getenv read of a GM_* name must
    be added here WITH its test, or this fails."""
    import glob
    import re
    root = os.path.join(os.path.dirname(HERE), "generative_models_amd")
    files = glob.glob(os.path.join(root, "*.py")) + glob.glob(os.path.join(root, "csrc", "*"))
    found = set()
    for f in files:
        if f.endswith((".o", ".so")):
            continue
        found |= set(re.findall(r"(?:getenv|environ\.get|environ\[)\(?\"(GM_[A-Z0-9_]+)", open(f, errors="ignore").read()))
    steering = {   # switch -> the agreement test that covers both of its arms
        "GM_CAPTURED_GENERAL": "test_captured_general_path_equals_the_host_loop",
        "GM_DP_COMM": "test_dp_launch_structure_single_rank_rccl",
        "GM_RCCL_IN_GRAPH": "test_dp_launch_structure_single_rank_rccl",
        "GM_DP_PUSH": "GM_DP_PUSH",
        "GM_DP_ONE_KERNEL": "GM_DP_ONE_KERNEL",
        "GM_FOLD_HEAD": "test_summation_order_switches_agree_within_rounding",
        "GM_FOLD_HEAD_TP": "test_summation_order_switches_agree_within_rounding",
        "GM_WGP_STACK": "test_summation_order_switches_agree_within_rounding",
        "GM_WGP_PEN_IN_HEAD": "test_summation_order_switches_agree_within_rounding",
        "GM_DRA_STACK": "test_summation_order_switches_agree_within_rounding",
        "GM_PACKED": "test_fp32_resident_dataset_equals_bit_packed",
        "GM_PACKED_OPERAND": "test_packed_operand_rows_equal_fp32_rows",
        "GM_PIPELINE_EPOCHS": "test_epochs_enqueued_ahead_of_the_loss_read_back_change_nothing",
        "GM_RING": "test_small_ring_wraps_many_times_and_changes_nothing",
        "GM_GRAPH_ITERS": "test_graph_size_changes_nothing",
    }
    # not steering the arithmetic: where the library is, host threads, tracing, one test hook of the numpy restatement
    infrastructure = {"GM_LIB_PATH", "GM_HOST_THREADS", "GM_NUMPY_THREADS", "GM_KEEP_THREADS", "GM_TRACE_RUN",
                      "GM_TRACE_NOSYNC", "GM_NUMPY_SCALAR"}
    assert len(steering) <= 15
    assert found == set(steering) | infrastructure, (sorted(found - set(steering) - infrastructure),
                                                     sorted((set(steering) | infrastructure) - found))
    tests_text = "".join(open(f).read() for f in glob.glob(os.path.join(HERE, "test_*.py")) if not f.endswith("test_host_cpu.py"))
    for sw, needle in steering.items():
        assert sw in tests_text and needle in tests_text, (sw, needle)
