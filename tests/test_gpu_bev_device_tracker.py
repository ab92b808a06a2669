"""BEV(-t --device_tracker) against BEV(-t) on a short synthetic clip (the clip and weights of test_bev_temporal_and_render, rebuilt
here): equal track ids and every returned array equal bit for bit; and tracking.smooth_batch on a two-frame forward_batch against
the same two frames taken one at a time."""
import numpy as np
import pytest
import torch

from oracle import bev_oracle as BO
from oracle import romp_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    from romp_amd import lib
    lib.load()
    return torch.device('cuda:0')


def _model(flags):
    from romp_amd import bev
    s = bev.bev_settings(flags)
    s.GPU, s.center_thresh, s.max_batch = 0, 0.9995, 2
    return bev.BEV(s, state_dict=BO.make_bev_state_dict(0), smpla_model=O.make_synthetic_smpl(0, 11), smil_model=O.make_synthetic_smpl(5, 10))


def _clip(model, dev, frames=4):
    from romp_amd.utils import img_preprocess_device
    rs = np.random.RandomState(2)
    frame0 = rs.randint(0, 256, (360, 640, 3)).astype(np.uint8)
    for thresh in (0.9995, 0.999, 0.99, 0.9, 0.5, 0.1):                     # the highest threshold that still sees a few persons
        model.model.centermap_parser.conf_thresh = thresh
        probe = model.model(img_preprocess_device(frame0, dev)[0])
        if probe is not None and probe['cam'].shape[0] >= 3:
            break
    return thresh, [np.clip(frame0.astype(np.int32) + rs.randint(-5, 6, frame0.shape), 0, 255).astype(np.uint8) for _ in range(frames)]


def test_device_tracker_flag():
    from romp_amd import bev
    assert bev.bev_settings(['-t']).device_tracker is False and bev.bev_settings(['-t', '--device_tracker']).device_tracker is True


def test_clip_with_and_without_device_tracker(dev):
    from romp_amd import tracker
    tracker.Track.last_id = 0
    host, devi = _model(['-t']), _model(['-t', '--device_tracker'])
    assert hasattr(host, 'tracker') and not hasattr(devi, 'tracker') and not hasattr(host, 'device_smoothers')
    devi.model = host.model        # ONE network program for both: two instances may choose different (equally valid) conv variants
    thresh, clip = _clip(host, dev)
    seen = 0
    for f, frame in enumerate(clip):
        a, b = host(frame), devi(frame)
        assert a is not None and b is not None
        assert sorted(a) == sorted(b)
        assert a['track_ids'].dtype == b['track_ids'].dtype and np.array_equal(a['track_ids'], b['track_ids'])
        for k in a:
            assert isinstance(b[k], type(a[k])), k
            if isinstance(a[k], np.ndarray):
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (f, k)
        seen += len(a['track_ids'])
    print('center threshold', thresh, 'tracked persons over the clip', seen)
    assert seen >= 3 * len(clip)


def test_smooth_batch_equals_frame_by_frame(dev):
    from romp_amd.tracking import TrackedSmoother, smooth_batch
    from romp_amd.utils import img_preprocess_device
    model = _model([])
    thresh, clip = _clip(model, dev, frames=2)
    images = torch.cat([img_preprocess_device(fr, dev)[0] for fr in clip])
    out = model.forward_batch(images)
    bids = out['pred_batch_ids']
    N = bids.shape[0]
    assert out is not None and set(bids.tolist()) == {0, 1}
    both = smooth_batch(TrackedSmoother(dev, 3., out['smpl_betas'].shape[1], 64), out)
    single = TrackedSmoother(dev, 3., out['smpl_betas'].shape[1], 64)
    parts = []
    for b in (0, 1):                                                          # the same detections, one frame per call
        sel = bids == b
        part = smooth_batch(single, {k: (v[sel] if torch.is_tensor(v) and v.shape[:1] == (N,) else v) for k, v in out.items()})
        assert part is not None
        parts.append(part)
    assert both is not None and sorted(both) == sorted(parts[0])
    for k in both:
        if k == 'track_ids':
            assert np.array_equal(both[k], np.concatenate([p[k] for p in parts]))
        elif torch.is_tensor(both[k]) and both[k].shape[:1] == (len(both['track_ids']),):
            assert torch.equal(both[k], torch.cat([p[k] for p in parts])), k
    assert len(both['track_ids']) >= 6 and both['pred_batch_ids'].tolist() == sorted(both['pred_batch_ids'].tolist())
