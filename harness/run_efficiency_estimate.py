#!/usr/bin/env python3
"""Counterpart of the reference's ``Signal_vs_Noise/Efficiency_test/src/calculate_efficiencies.py`` on the MI355X path.

    run_efficiency_estimate.py [i_run | i_run_first i_run_last] [flags]

For every (run, epoch) it loads ``lora_weights_run_%04i_epoch_%04i.pt`` (``PeftModel.from_pretrained``) and
``dense_layers_run_%04i_epoch_%04i.pth`` from ``--state-dicts-dir`` (``calculate_efficiencies.py:65-78``), replaces the
Softmax by the logit-difference layer unless ``--keep-softmax`` (``:93-106``; ``--remove-softmax`` is the default), runs
``EfficiencyEstimator`` over the test split's injections and pure noise (``:59-63``) and writes
``<output-directory>/out_efficiencies_run_%04i_epoch_%04i.txt`` in the reference's text format (``:84-114``).  Defaults as
there: ``--snrs 5 7 ... 23``, ``--faps 0.1 0.01 0.001 0.0001 0.00001``, test signals / combined noises ``0 100000``, pure
noises ``0 400000``; the reference's hard-wired epoch list ``[40, 55, 70]`` is ``--epochs-list``.

Differences that come with the hardware path: the whole estimate stays on the device (scores into one buffer, radix
selection of the thresholds, counts accumulated per SNR, ONE read of the table); the estimator's batch size is
``--batch-size`` (default 256; the reference's DataLoader default is 16) and does not change the table; data files, the
encoder weights and ``--synthetic`` as in run_efficiency_train.py.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from run_efficiency_train import add_data_flags  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="Detection-efficiency estimation (MI355X path)")
    p.add_argument("runs", type=int, nargs="*", help="nothing: range(runs_number); one: that run; two: range(first, last)")
    add_data_flags(p)
    p.add_argument("--test-prefix", type=str, default="thr_")
    p.add_argument("--test-noises-per-signal", type=int, default=1)
    p.add_argument("--test-signals", type=int, nargs=2, default=[0, 100000])
    p.add_argument("--test-combined-noises", type=int, nargs=2, default=[0, 100000])
    p.add_argument("--test-pure-noises", type=int, nargs=2, default=[0, 400000])
    p.add_argument("--epochs-list", type=int, nargs="+", default=[40, 55, 70])
    p.add_argument("--snrs", type=float, nargs="+", default=[float(s) for s in np.arange(5, 25, 2)])
    p.add_argument("--faps", type=float, nargs="+", default=[0.1, 0.01, 0.001, 0.0001, 0.00001])
    p.add_argument("--remove-softmax", dest="remove_softmax", action="store_true", default=True)
    p.add_argument("--keep-softmax", dest="remove_softmax", action="store_false")
    p.add_argument("--batch-size", type=int, default=256)
    p.add_argument("--output-directory", type=str, default="Detection/Efficiency_test/src/efficiencies")
    return p


def main(args):
    from gw_whisper_amd import efficiency
    assert torch.cuda.is_available(), "run_efficiency_estimate.py needs an MI355X (gw_whisper_amd has no CPU path)"
    device = torch.device("cuda", 0)
    if len(args.runs) == 0:
        indices_run = range(args.runs_number)
    elif len(args.runs) == 1:
        indices_run = [args.runs[0]]
    elif len(args.runs) == 2:
        indices_run = range(args.runs[0], args.runs[1])
    else:
        raise ValueError
    print("indices_run = %s" % str(indices_run), flush=True)
    if args.synthetic:
        n = args.synthetic
        wave, noise = efficiency.synthetic_tensors(n, 5 * n, seed=args.seed + 7919 * 2)
        test = efficiency.ResampledDataset(torch.from_numpy(wave).to(device), torch.from_numpy(noise).to(device), (0, 0),
                                           (0, n), (0, n), (0, 5 * n), seed=args.seed)
    else:
        ia = [args.test_noises_per_signal, args.test_signals, args.test_combined_noises, args.test_pure_noises]
        test = efficiency.load_resampled_dataset(args.path, args.test_prefix + args.waveform_fname,
                                                 args.test_prefix + args.noise_fname, (0, 0), ia, device=device, seed=args.seed)
    wave_ds = efficiency.ResampledDataset(test.wave_tensor, test.noise_tensor, (0., 0.), test.wave_lim, test.noise_comb_lim,
                                          (0, 0), noises_per_signal=test.noises_per_signal)
    noise_ds = efficiency.ResampledDataset(test.wave_tensor, test.noise_tensor, (0., 0.), (0, 0), (0, 0), test.noise_pure_lim,
                                           noises_per_signal=test.noises_per_signal)
    estimator = efficiency.EfficiencyEstimator(wave_ds, noise_ds, args.snrs, batch_size=args.batch_size, faps=args.faps)
    os.makedirs(args.output_directory, exist_ok=True)
    for i_run in indices_run:
        for e in args.epochs_list:
            lora = os.path.join(args.state_dicts_dir, "lora_weights_run_%04i_epoch_%04i.pt" % (i_run, e))
            dense = os.path.join(args.state_dicts_dir, "dense_layers_run_%04i_epoch_%04i.pth" % (i_run, e))
            print(lora, flush=True)
            network = efficiency.build_model("tiny", 2, precision=args.precision, encoder_weights=args.encoder_weights,
                                             seed=args.seed, device=device, adapter_path=lora)
            network.classifier.load_state_dict(torch.load(dense, map_location=device))
            network.eval()
            if args.remove_softmax:
                efficiency.remove_softmax(network)
            table = estimator(network)
            with open(os.path.join(args.output_directory, "out_efficiencies_run_%04i_epoch_%04i.txt" % (i_run, e)), "w") as f:
                f.write(efficiency.efficiency_text(args.faps, args.snrs, table))


if __name__ == "__main__":
    main(build_parser().parse_args())
