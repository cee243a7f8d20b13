"""TimeLapseImaging — apis/timeLapseImaging.py:22-211 on the device.

Mirrors the reference class's constructor, attributes and imaging methods:
  _preprocessing_for_surface_waves  :50-71   bandpass + empty / noisy trace imputation + trace norm
                                             (preprocess.surface_wave_preprocessing, dvh_sosfiltfilt,
                                             dvh_trace_cleanup)
  preprocess_for_tracking           :73-104  _preprocess_for_tracking: median gate, imputation, 0.08-1 Hz
                                             bandpass, 204/25 resampling onto the 1 m x 50 Hz tracking grid,
                                             spatial bandpass (preprocess.tracking_preprocessing,
                                             dvh_median_abs_gate, dvh_resample_rows_t, dvh_transpose_f64)
  select_surface_wave_windows       :166-196 SurfaceWaveSelector on data_for_imaging (sw_selector)
                                             and on the raw data (qs_selector), cut on the device
  get_images                        :198-201 DispersionImagesFromWindows (flavour B) or
                                             VirtualShotGathersFromWindows (xcorr) of sw_selector
  save_avg_disp_to_npz              :205-206
  track_vehicles                    :104-119 track_cars without its plot: KF_tracking of this package
                                             (apis/tracking.py: dvh_find_peaks_rows, dvh_peak_likelihood,
                                             dvh_kf_track) on data_for_tracking, which stays on the device
The constructor skips the tracking preprocessing (unlike the reference's); the flow from a raw record is

  obj = TimeLapseImaging(data, x_axis, t_axis)
  obj.track_vehicles(start_x, end_x)                 # preprocess_for_tracking() if needed, then veh_states
  obj.select_surface_wave_windows(x0)

``track_cars`` itself (whose default draws the detection plot) still raises.  Tracks made elsewhere are attached
with ``set_veh_states`` (on the grid left by preprocess_for_tracking) or, with their own grid (e.g. the reference's
tracker run on the CPU, or stored tracks), with ``set_tracking``.
"""
from __future__ import annotations

import numpy as np

from ..preprocess import surface_wave_preprocessing, tracking_preprocessing
from .data_classes import SurfaceWaveSelector
from .imaging_classes import DispersionImagesFromWindows, VirtualShotGathersFromWindows
from .tracking import KF_tracking

# apis/imaging_workflow.py:14-20
DEFAULT_TRACKING_PARAM = {"detect": {"minprominence": 0.2, "minseparation": 50, "prominenceWindow": 600}}

channel_prop = {"odh3": {"start_ch": 400, "dx": 8.16}}  # apis/timeLapseImaging.py:14-19


class TimeLapseImaging:
    def __init__(self, data, x_axis, t_axis, interrogator="odh3", method="surface_wave",
                 tracking_preprecessing_dict=None, surface_wave_preprecessing_dict=None):
        assert method in {"surface_wave", "xcorr"}
        self.method = method
        prop = channel_prop[interrogator]
        self.data = data
        self.t_axis = t_axis
        self.dt = self.t_axis[1] - self.t_axis[0]
        self.x_axis = x_axis
        self.start_ch = prop["start_ch"]
        self.dx = prop["dx"]
        self.distances_along_fiber = (x_axis - self.start_ch) * self.dx
        self.tracking_preprecessing_dict = tracking_preprecessing_dict if tracking_preprecessing_dict is not None else {}
        self.surface_wave_preprecessing_dict = surface_wave_preprecessing_dict
        self._preprocessing_for_surface_waves()

    def _preprocessing_for_surface_waves(self, impute_noise_traces=True, noise_threshold=5, impute_empty_traces=True):
        if self.surface_wave_preprecessing_dict is None:
            self.surface_wave_preprecessing_dict = {}
        flo = self.surface_wave_preprecessing_dict.get("flo", 1.2)
        fhi = self.surface_wave_preprecessing_dict.get("fhi", 30)
        self.data_for_imaging = surface_wave_preprocessing(
            self.data, self.dt, method=self.method, flo=flo, fhi=fhi, impute_noise_traces=impute_noise_traces,
            noise_threshold=noise_threshold, impute_empty_traces=impute_empty_traces)

    def preprocess_for_tracking(self, subsamp_factor=5, noise_level=10, channel0=400):
        """_preprocess_for_tracking (:74-102) on the device; explicit, the constructor does not call it."""
        d = self.tracking_preprecessing_dict
        self.data_for_tracking, self.dist_along_fiber_tracking, step = tracking_preprocessing(
            self.data, self.dt, self.x_axis[0], flo=d.get("flo", 0.08), fhi=d.get("fhi", 1),
            flo_space=d.get("flo_space", 0.006), fhi_space=d.get("fhi_space", 0.04), subsamp_factor=subsamp_factor,
            noise_level=noise_level, channel0=channel0)
        self.t_axis_tracking = self.t_axis[::step]

    def set_tracking(self, veh_states, start_x, dist_along_fiber_tracking, t_axis_tracking, end_x=None):
        """The attributes track_cars / _preprocess_for_tracking leave behind (:73-120)."""
        self.veh_states = np.asarray(veh_states)
        self.start_x = start_x
        self.end_x = end_x
        self.dist_along_fiber_tracking = np.asarray(dist_along_fiber_tracking)
        self.t_axis_tracking = np.asarray(t_axis_tracking)

    def set_veh_states(self, veh_states, start_x, end_x=None):
        """The attributes track_cars leaves behind (:105-119), for tracks made on the grid of
        preprocess_for_tracking."""
        if not hasattr(self, "dist_along_fiber_tracking") or not hasattr(self, "t_axis_tracking"):
            raise AttributeError("no tracking grid: call preprocess_for_tracking() first (or set_tracking())")
        self.veh_states = np.asarray(veh_states)
        self.start_x = start_x
        self.end_x = end_x

    def track_vehicles(self, start_x, end_x, tracking_args=None, reverse_amp=True, sigma_a=0.01):
        """track_cars (:104-119) without the plot: detection over the 15 rows from start_x (sigma = 0.08), then the
        tracks of every third row up to end_x.  The grid stays on the device and is not negated: reverse_amp is the
        sign the peak picking applies on load.  tracking_args=None takes DEFAULT_TRACKING_PARAM."""
        if not hasattr(self, "data_for_tracking"):
            self.preprocess_for_tracking()
        self.start_x = start_x
        self.end_x = end_x
        self.tracking_args = tracking_args if tracking_args else DEFAULT_TRACKING_PARAM
        self.tracking = KF_tracking(data=self.data_for_tracking, t_axis=self.t_axis_tracking,
                                    x_axis=self.dist_along_fiber_tracking, args=self.tracking_args,
                                    sign=-1 if reverse_amp else 1)
        veh_base = self.tracking.detect_in_one_section(start_x=self.start_x, nx=15, sigma=0.08)
        self.veh_states = self.tracking.tracking_with_veh_base(start_x=self.start_x, end_x=self.end_x,
                                                               veh_base=veh_base, sigma_a=sigma_a)
        return self.veh_states

    def track_cars(self, *args, **kwargs):
        raise NotImplementedError("track_cars draws the detection plot; track_vehicles(start_x, end_x, tracking_args) "
                                  "tracks on the device without it (or attach tracks with set_tracking())")

    def select_surface_wave_windows(self, x0, **kwargs):
        if not hasattr(self, "veh_states"):
            raise AttributeError("no vehicle tracks: call track_vehicles() or set_tracking() first")
        args = (self.distances_along_fiber, self.t_axis, x0, self.start_x, self.veh_states,
                self.dist_along_fiber_tracking, self.t_axis_tracking)
        self.sw_selector = SurfaceWaveSelector(self.data_for_imaging, *args, **kwargs)
        self.qs_selector = SurfaceWaveSelector(self.data, *args, **kwargs)

    def get_images(self, mute_offset=300, **imaging_kwargs):
        cls = DispersionImagesFromWindows if self.method == "surface_wave" else VirtualShotGathersFromWindows
        self.images = cls(self.sw_selector)
        self.images.get_images(mute_offset=mute_offset, **imaging_kwargs)

    def save_avg_disp_to_npz(self, *args, fdir=".", **kwargs):
        self.images.avg_image.save_to_npz(*args, fdir=fdir, **kwargs)
