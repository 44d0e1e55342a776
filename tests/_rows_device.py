"""What the bin-by-bin GPU modules (tests/test_gpu_rows.py, tests/test_gpu_pairs.py) share: the form switches the launcher
reads per launch, a case's plan, a stream on the device."""
import numpy as np

import _rows_cases as K

ENV = ("GLFER_FORM", "GLFER_Y_TAPERS", "GLFER_MEAN_PREPASS")


def _select(monkeypatch, form):
    """default | h | w | x (GLFER_FORM) | full (GLFER_Y_TAPERS) | prepass (GLFER_MEAN_PREPASS=1); each read per launch."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if form in ("h", "w", "x"):
        monkeypatch.setenv("GLFER_FORM", form)
    elif form == "full":
        monkeypatch.setenv("GLFER_Y_TAPERS", "full")
    elif form == "prepass":
        monkeypatch.setenv("GLFER_MEAN_PREPASS", "1")
    else:
        assert form == "default", form


def _plan(lib, oracle, c, sub_mean=None, **kw):
    """The case's plan; its float32 window / double tapers are the ones the float64 rows were made with."""
    fmt = {"f32": lib.SAMPLES_F32, "s16": lib.SAMPLES_S16, "u8": lib.SAMPLES_U8}[c.fmt]
    m = c.sub_mean if sub_mean is None else sub_mean
    if c.est == "fft":
        sp = lib.Spectrogram(lib.FftParams(n=c.n, window_type=lib.WINDOWS[c.window], overlap=c.ovl, sub_mean=m,
                                           history_mode=c.history_mode, sample_format=fmt, **kw))
        assert np.array_equal(sp.window(), oracle.window(oracle.WINDOWS[c.window], c.n))
    else:
        sp = lib.Spectrogram(lib.MtmParams(n=c.n, overlap=c.ovl, w=c.nw, kmax=c.kmax, sub_mean=m, history_mode=c.history_mode,
                                           sample_format=fmt, **kw))
        v, sig = sp.tapers()
        ov, osig = K.tapers(oracle, c.n, c.kmax, c.nw)
        assert np.array_equal(v, ov) and np.array_equal(sig, osig)
    return sp


def _upload(torch, raw, offset=0):
    """The stream on the device; offset > 0: that many samples into its allocation."""
    if not offset:
        return torch.from_numpy(raw).cuda()
    host = np.concatenate([np.full(offset, 77, raw.dtype), raw])
    return torch.from_numpy(host).cuda()[offset:]
