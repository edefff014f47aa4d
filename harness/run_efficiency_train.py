#!/usr/bin/env python3
"""Counterpart of the reference's ``Signal_vs_Noise/Efficiency_test/src/train.py`` on the MI355X path.

    run_efficiency_train.py [i_run_init] [flags]

The reference has no command line beyond ``i_run_init``: its settings are the module-level names of ``pars.py`` and
``scheduler_pars.py``, and the flags here carry those names (``--lr``, ``--batch-size``, ``--epochs``, ``--runs-number``,
the six index ranges and the ``*-noises-per-signal`` values, ``--final-snr-range``, ``--initial-snr-range``,
``--snr-steps``, ``--cl-scheduler``) with the same defaults.  Same construction sequence (``train.py:52-102``:
whisper-tiny encoder -> fnmatch search for ``k_proj`` / ``v_proj`` -> ``LoraConfig(use_dora=True, r=8, lora_alpha=32)`` ->
``get_peft_model`` -> ``requires_grad = 'lora' in name`` -> the 2-way Softmax head -> ``reg_BCELoss(dim=2,
epsilon=1e-6)`` + ``Adam(Network.parameters(), lr)`` -> the curriculum scheduler over the train and validation datasets,
reloading the optimizer on every range change), same loop (``:112-188``: shuffled training batches with the last partial
batch kept, ``train_loss`` and ``valid_loss`` the mean of the per-batch mean losses, validation in shuffled batches of 32,
accuracy by argmax) and the same artefacts: ``<outfiles-dir>/out_train_%04i.txt`` with lines
``'%04i    %1.12e    %1.12e    %f\\n'``, and under ``<state-dicts-dir>`` ``state_dict_run_%04i_epoch_%04i.pt``,
``optim_state_dict_run_%04i_epoch_%04i.pt``, ``lora_weights_run_%04i_epoch_%04i.pt`` (a ``save_pretrained`` directory),
``dense_layers_run_%04i_epoch_%04i.pth`` (keys ``0 2 4 6 8``), the ``best_state_dict_%04i.pt`` / ``best_lora_weights_run_`` /
``best_dense_layers_run_`` set once the scheduler is done, and the ``final_`` set.

Differences that come with the hardware path:
  * the datasets live in HBM at 16 kHz and a batch is assembled and turned into log-mel features on the device
    (``efficiency.ResampledDataset.batch``); the SNR draws and the shuffles are seeded (``--seed``);
  * ``--head hip`` runs the head, its Softmax, the loss and their backward as four HIP launches
    (``efficiency.reg_bce_head``), keeps the training loss on the device and reads it once per epoch, and validates with
    the device accumulate (one read per epoch); ``--head torch`` is the reference's ``nn.Sequential`` + ``RegBCELoss`` with
    ``loss.item()`` per batch and a per-batch argmax compare.  The default is the one profiles/efficiency_train.md
    measured as not slower;
  * files are HDF5 (``data/0``) when ``h5py`` is importable, otherwise ``.npz`` twins of the same layout;
    ``--synthetic N`` replaces them by N seeded chirps and 2 N seeded noise segments per split;
  * pretrained ``openai/whisper-tiny`` weights cannot be downloaded here: ``--encoder-weights`` takes a HF encoder
    ``state_dict`` (.pth / .safetensors), otherwise seeded random weights.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEFAULT_HEAD = "hip"


def load_splits(args, device):
    from gw_whisper_amd import efficiency
    if args.synthetic:
        n = args.synthetic
        out = []
        for k in range(2):
            wave, noise = efficiency.synthetic_tensors(n, 2 * n, seed=args.seed + 7919 * k)
            out.append(efficiency.ResampledDataset(torch.from_numpy(wave).to(device), torch.from_numpy(noise).to(device),
                                                   (5, 15), (0, n), (0, n), (n, 2 * n), seed=args.seed + k))
        return out
    arrays = ((args.train_prefix, [args.train_noises_per_signal, args.train_signals, args.train_combined_noises,
                                   args.train_pure_noises]),
              (args.valid_prefix, [args.valid_noises_per_signal, args.valid_signals, args.valid_combined_noises,
                                   args.valid_pure_noises]))
    # train.py:36, 40: the range given at load is (5, 15); the scheduler sets the first real one
    return [efficiency.load_resampled_dataset(args.path, prefix + args.waveform_fname, prefix + args.noise_fname, (5, 15),
                                              ia, device=device, seed=args.seed + k)
            for k, (prefix, ia) in enumerate(arrays)]


def make_scheduler(args, datasets, opt):
    from gw_whisper_amd import efficiency
    ranges = efficiency.snr_ranges(args.initial_snr_range or args.final_snr_range, args.final_snr_range, args.snr_steps)
    cls = {"plateau": efficiency.PlateauCLScheduler, "threshold": efficiency.ThresholdCLScheduler,
           "epoch": efficiency.EpochCLScheduler}[args.cl_scheduler]
    kwargs = {}
    if args.cl_patience is not None and args.cl_scheduler != "threshold":
        kwargs["patience"] = args.cl_patience
    if args.cl_threshold is not None and args.cl_scheduler != "epoch":
        kwargs["threshold"] = args.cl_threshold
    return cls(ranges, datasets, optim=opt, **kwargs)


def save_models(results_path, peft_model, dense_layers, lora_weights_path, dense_layers_path):     # train.py:204-212
    peft_model.save_pretrained(os.path.join(results_path, lora_weights_path))
    torch.save(dense_layers.state_dict(), os.path.join(results_path, dense_layers_path))


def run_training(args, i_run, train_ds, valid_ds, device):
    from gw_whisper_amd import efficiency, inference, ops
    from gw_whisper_amd.models import _pooled
    crit = inference.RegBCELoss(dim=2, epsilon=1.e-6)
    tr_outfile = open(os.path.join(args.outfiles_dir, "out_train_%04i.txt" % i_run), "w", buffering=1)
    torch.manual_seed(args.seed + i_run)             # peft's lora_A and the head's initialisation
    network = efficiency.build_model("tiny", 2, 8, 32, args.precision, args.encoder_weights, args.seed, device)
    opt = torch.optim.Adam(network.parameters(), lr=args.lr)
    sched = make_scheduler(args, (train_ds, valid_ds), opt)
    rng = np.random.default_rng(args.seed + 104729 * (i_run + 1))
    sd_dir = args.state_dicts_dir
    min_valid_loss = 1.e100
    for e in range(1, args.epochs + 1):
        network.train()
        losses = []
        order = rng.permutation(len(train_ds))                                    # DataLoader(shuffle=True)
        for i in range(0, len(order), args.batch_size):
            mel, targets, _ = train_ds.batch(order[i:i + args.batch_size])
            opt.zero_grad()
            if args.head == "hip":
                loss, _ = efficiency.reg_bce_head(network.classifier, _pooled(network.encoder, mel), targets, 1.e-6)
                loss.backward()
                losses.append(loss.detach())                                       # read once per epoch
            else:
                loss = crit(network(mel).float(), targets)
                loss.backward()
                losses.append(loss.detach().item())                                # train.py:127
            opt.step()
        if losses and torch.is_tensor(losses[0]):
            losses = torch.stack(losses).double().cpu().tolist()
        train_loss = float(np.sum(losses)) / max(len(losses), 1)
        with torch.no_grad():
            network.eval()
            order = rng.permutation(len(valid_ds))
            if args.head == "hip":
                state = efficiency.EvalState(device)
                params = [t.detach() for t in efficiency._det_parameters(network.classifier)]
                for i in range(0, len(order), 32):
                    mel, targets, _ = valid_ds.batch(order[i:i + 32])
                    _, _, probs, row_loss, _ = ops.det_head_forward(_pooled(network.encoder, mel).to(torch.float32), params,
                                                                    targets, 1.e-6)
                    state.add(probs, targets, row_loss)
                valid_loss, valid_accuracy, _, _ = state.read()                    # ONE read
            else:
                valid_loss, samples, valid_accuracy, batches = 0., 0, 0, 0
                for i in range(0, len(order), 32):
                    mel, targets, _ = valid_ds.batch(order[i:i + 32])
                    outputs = network(mel).float()
                    valid_loss += crit(outputs, targets).detach().item()
                    batches += 1
                    samples += len(targets)
                    valid_accuracy += int((torch.argmax(targets, 1) == torch.argmax(outputs, 1)).sum().item())
                valid_loss /= batches
                valid_accuracy /= samples
        tr_outfile.write("%04i    %1.12e    %1.12e    %f\n" % (e, train_loss, valid_loss, valid_accuracy))
        print("Epoch %04i training loss: %1.12e validation loss: %1.12e, accuracy: %f" % (e, train_loss, valid_loss,
                                                                                          valid_accuracy), flush=True)
        if sched.done and valid_loss < min_valid_loss:
            torch.save(network.state_dict(), os.path.join(sd_dir, "best_state_dict_%04i.pt" % i_run))
            min_valid_loss = valid_loss
            save_models(sd_dir, network.encoder, network.classifier, "best_lora_weights_run_%04i.pt" % i_run,
                        "best_dense_layers_run_%04i.pth" % i_run)
        torch.save(network.state_dict(), os.path.join(sd_dir, "state_dict_run_%04i_epoch_%04i.pt" % (i_run, e)))
        torch.save(opt.state_dict(), os.path.join(sd_dir, "optim_state_dict_run_%04i_epoch_%04i.pt" % (i_run, e)))
        save_models(sd_dir, network.encoder, network.classifier, "lora_weights_run_%04i_epoch_%04i.pt" % (i_run, e),
                    "dense_layers_run_%04i_epoch_%04i.pth" % (i_run, e))
        sched.step(valid_loss, valid_accuracy)
        if sched.interrupt:
            break
    save_models(sd_dir, network.encoder, network.classifier, "final_lora_weights_run_%04i.pt" % i_run,
                "final_dense_layers_run_%04i.pth" % i_run)
    tr_outfile.close()


def add_data_flags(p):
    """The names of pars.py that both programs share."""
    p.add_argument("--path", type=str, default="Detection/Efficiency_test/data")
    p.add_argument("--waveform-fname", type=str, default="signals.hdf")
    p.add_argument("--noise-fname", type=str, default="noise.hdf")
    p.add_argument("--runs-number", type=int, default=1)
    p.add_argument("--outfiles-dir", type=str, default="Detection/Efficiency_test/src/outfiles")
    p.add_argument("--state-dicts-dir", type=str, default="Detection/Efficiency_test/src/state_dicts")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--synthetic", type=int, default=0, help="N seeded chirps and 2 N seeded noise segments per split, no files")
    p.add_argument("--encoder-weights", type=str, default=None, help="HF WhisperEncoder state_dict (.pth / .safetensors)")
    p.add_argument("--precision", choices=("bf16", "fp32"), default="bf16", help="encoder arithmetic")


def build_parser():
    p = argparse.ArgumentParser(description="Efficiency-test training (MI355X path)")
    p.add_argument("i_run_init", type=int, nargs="?", default=0)
    add_data_flags(p)
    p.add_argument("--train-prefix", type=str, default="train_")
    p.add_argument("--valid-prefix", type=str, default="val_")
    p.add_argument("--lr", type=float, default=0.0001)
    p.add_argument("--batch-size", type=int, default=32)
    p.add_argument("--epochs", type=int, default=75)
    for split in ("train", "valid"):
        p.add_argument(f"--{split}-noises-per-signal", type=int, default=1)
        p.add_argument(f"--{split}-signals", type=int, nargs=2, default=[0, 100000])
        p.add_argument(f"--{split}-combined-noises", type=int, nargs=2, default=[0, 100000])
        p.add_argument(f"--{split}-pure-noises", type=int, nargs=2, default=[100000, 200000])
    p.add_argument("--final-snr-range", type=float, nargs=2, default=[5., 15.])
    p.add_argument("--initial-snr-range", type=float, nargs=2, default=None, help="default: the final range")
    p.add_argument("--snr-steps", type=int, default=0)
    p.add_argument("--cl-scheduler", choices=("plateau", "threshold", "epoch"), default="plateau")
    p.add_argument("--cl-patience", type=int, default=None, help="the scheduler's patience (its own default: 4)")
    p.add_argument("--cl-threshold", type=float, default=None, help="the scheduler's threshold (its own default)")
    p.add_argument("--head", choices=("hip", "torch"), default=DEFAULT_HEAD,
                   help="head + loss: the HIP head step or torch.nn (profiles/efficiency_train.md)")
    return p


def main(args):
    assert torch.cuda.is_available(), "run_efficiency_train.py needs an MI355X (gw_whisper_amd has no CPU path)"
    device = torch.device("cuda", 0)
    os.makedirs(args.outfiles_dir, exist_ok=True)
    os.makedirs(args.state_dicts_dir, exist_ok=True)
    train_ds, valid_ds = load_splits(args, device)
    for i_run in range(args.i_run_init, args.i_run_init + args.runs_number):
        run_training(args, i_run, train_ds, valid_ds, device)


if __name__ == "__main__":
    main(build_parser().parse_args())
