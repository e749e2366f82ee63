"""CPU oracle of the pipeline's two-view bootstrap (vo_pipeline_bootstrap_seq): vo.driver.bootstrap's steps
(src/main.py:204-230) composed from what is pinned already --

  * oracle.native.good_features / klt_track (oracle/csrc goodfeatures.c, klt.c) for corners and LK,
  * oracle.bootstrap_np.find_fundamental_matrix_ransac_px / find_relative_pose for the 8-point RANSAC of the
    use_opencv=True route and the cheirality vote,
  * the bookkeeping classes of vo.primitives (Features / Frame / Matches / State, pinned by tests/golden/bookkeeping.npz)
    in the order vo.driver.bootstrap calls them.

TEST INFRASTRUCTURE ONLY: nothing here touches the GPU."""
import numpy as np

from oracle import bootstrap_np, native


def bootstrap(img_a, img_b, K, max_corners=500, quality=0.01, min_distance=8, block=7, win=17, max_level=2, max_iter=10,
              eps=0.03, min_eig=1e-4, err_threshold=100, threshold_px=0.25, outlier_ratio=0.9, confidence=0.999,
              max_iterations=2000):
    """dict(features (of frame b), curr_pose, prev_pose, M, X, ransac_inliers, mask, n_corners, n_tracked, num_features,
    iterations)."""
    from vo.primitives import Features, Frame, Matches, State
    K = np.asarray(K, np.float64)
    # klt.py:87-115 + 191-280 for a first frame: corners, LK, keep status & err < threshold, identity pairs
    corners = native.good_features(img_a, None, max_corners, quality, min_distance, block).reshape(-1, 2, 1)
    frame_a = Frame(img_a, features=Features(keypoints=corners))
    nxt, status, err = native.klt_track(img_a, img_b, corners.reshape(-1, 2), win=win, max_level=max_level, max_iter=max_iter,
                                        eps=eps, min_eig=min_eig)
    keep = status.astype(bool) & (err < np.float32(err_threshold))
    frame_b = Frame(img_b, features=Features(keypoints=nxt.reshape(-1, 2, 1)))
    frame_b.features.mask(keep)
    frame_a.features.mask(keep)
    same = np.arange(frame_b.features.length).reshape(-1, 1)
    state = State(frame_a)
    matches = Matches(frame_a, frame_b, np.hstack((same, same)))
    state.update_from_matches(matches)
    # triangulation.py:88-163, 279-350 (triangulate_matches, use_opencv=True route)
    p1 = frame_a.features.matched_candidate_inliers_keypoints.astype(np.float64)
    p2 = frame_b.features.matched_candidate_inliers_keypoints.astype(np.float64)
    F, ransac_inliers, rs = bootstrap_np.find_fundamental_matrix_ransac_px(p1, p2, threshold_px, outlier_ratio, confidence,
                                                                           max_iterations)
    M, X, inliers, _ = bootstrap_np.find_relative_pose(p1, p2, K, K, F, ransac_inliers)
    # vo.driver.bootstrap after triangulate_matches (main.py:215-230)
    f2 = frame_b.features
    outliers = np.zeros(shape=(f2.length,), dtype=bool)
    outliers[f2.match_inliers] = ~inliers
    state.update_with_local_pose(M)
    inliers_mask = np.zeros_like(f2.matched_candidate_inliers).astype(bool)
    inliers_mask[f2.matched_candidate_inliers] = inliers
    state.update_with_local_landmarks(X[inliers], inliers_mask)
    state.reset_outliers(outliers)
    return dict(features=f2, curr_pose=state.curr_pose, prev_pose=state.prev_pose, M=M, X=X,
                ransac_inliers=np.asarray(ransac_inliers, bool), mask=np.asarray(inliers, bool), n_corners=corners.shape[0],
                n_tracked=int(keep.sum()), num_features=corners.shape[0], iterations=rs.iterations_done)


def pose_errors(M, T_wc_a, T_wc_b):
    """(rotation error in degrees, cosine between the translation directions) of M (camera a -> camera b, |t| = 1)
    against the analytic camera-to-world poses of the two frames."""
    T = np.linalg.inv(T_wc_b) @ T_wc_a
    dR = M[:3, :3] @ T[:3, :3].T
    ang = float(np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0))))
    a, b = M[:3, 3], T[:3, 3]
    return ang, float(a @ b / max(np.linalg.norm(a) * np.linalg.norm(b), 1e-30))


def check_invariants(features, curr_pose):
    """Step 4's end state: state 2 <=> finite landmark (track from the frame-a corner at the identity), no state 1, every
    other feature in state 0 tracking from its own keypoint at the current pose, no candidate."""
    st = np.asarray(features.state)
    land = np.asarray(features.landmarks).reshape(-1, 3)
    assert not np.any(st == 1)
    assert set(np.unique(st)) <= {0.0, 2.0}
    assert np.array_equal(st == 2, np.all(np.isfinite(land), axis=1))
    assert np.all(np.isnan(land[st == 0]))
    reset = st == 0
    assert np.array_equal(np.asarray(features.tracks)[reset], np.asarray(features.keypoints)[reset].astype(np.float64))
    assert np.allclose(np.asarray(features.poses)[reset], curr_pose, rtol=0, atol=1e-13)
    assert np.array_equal(np.asarray(features.poses)[~reset], np.stack([np.eye(4)] * int((~reset).sum())).reshape(-1, 4, 4))
    assert not np.any(features.candidate_mask)
